"""fg::band_cuts / fg::band_tier, the pure cut and tier-of-score rule of the
score-tiered lead copies (fg_internal.h; the build cuts each dense term's score
histogram with it and k_band_count / k_band_scatter place every posting by it),
checked against lists sorted by score -- all scores equal, two values, a class of
equal scores straddling a share, lengths 1, 2048 and 2049 -- by a stand-alone C++
program (tests/band_cuts_check.cpp) built with AddressSanitizer and UBSan and
run directly: no device, no library, nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_band_cuts_under_sanitizers(tmp_path):
    exe = tmp_path / "band_cuts_check"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{ROOT}/fugu_amd/csrc",
                    os.path.join(ROOT, "tests", "band_cuts_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "band_cuts ok" in out.stdout
