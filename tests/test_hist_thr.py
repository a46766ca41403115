"""fg::hist_kth_edge, the pure k-th edge rule of a query's score histogram
(fg_internal.h; hist_threshold and the threshold an ending k_conj item
publishes both use it), checked against the true k-th key of random items by a
stand-alone C++ program (tests/hist_thr_check.cpp) built with AddressSanitizer
and UBSan and run directly: no device, no library, nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_hist_kth_edge_under_sanitizers(tmp_path):
    exe = tmp_path / "hist_thr_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{ROOT}/fugu_amd/csrc",
                    os.path.join(ROOT, "tests", "hist_thr_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hist_kth_edge ok" in out.stdout
