"""The sampling part of a sequence's settings on the CPU: tests/c/seq_sampling_check.cc drives csrc/gvl_seq_table.h (no HIP) through new / fork / clone / reset /
close and checks who follows the default and who carries a setting of its own.  Built with the host C++ compiler; with AddressSanitizer and UBSan where the
compiler links them (a stand-alone program: nothing sanitised is loaded into Python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "seq_sampling_check.cc")


def _build(tmp_path, extra):
    exe = str(tmp_path / ("check" + ("_san" if extra else "")))
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pedantic", *extra, "-I", CSRC, SRC, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def test_seq_sampling_settings(tmp_path):
    exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1].startswith("passed ") and int(lines[-1].split()[1]) == len(lines) - 1 >= 15
    assert all(ln.startswith("ok ") for ln in lines[:-1])


def test_seq_sampling_settings_sanitized(tmp_path):
    """The same program under ASan + UBSan.  A toolchain without the sanitizer runtimes cannot link it: the plain run above is then the whole check."""
    exe, r = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr
        return
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines()[-1].startswith("passed ")
