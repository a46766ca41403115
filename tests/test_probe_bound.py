"""fg::probe_desc_bound, the planner's pure filler of the bound fields of
k_conj's clause-1 probe descriptor, and the u8 quantization of the bound tables
(quant8 / q8_bound, fg_internal.h), checked by a stand-alone C++ program
(tests/probe_bound_check.cpp) built with AddressSanitizer and UBSan and run
directly: no device, no library, nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_probe_bound_filler_and_quantization_under_sanitizers(tmp_path):
    exe = tmp_path / "probe_bound_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{ROOT}/fugu_amd/csrc",
                    os.path.join(ROOT, "tests", "probe_bound_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe_bound ok" in out.stdout
