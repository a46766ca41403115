"""fg::probe_desc, the planner's pure filler of k_conj's probe descriptors
(fg_internal.h), checked field by field on made-up addresses by a stand-alone
C++ program (tests/probe_desc_check.cpp) built with AddressSanitizer and
UBSan and run directly: no device, no library, nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_probe_desc_filler_under_sanitizers(tmp_path):
    exe = tmp_path / "probe_desc_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{ROOT}/fugu_amd/csrc",
                    os.path.join(ROOT, "tests", "probe_desc_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe_desc ok" in out.stdout
