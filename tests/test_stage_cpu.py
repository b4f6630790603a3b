"""The host-only parts of csrc/td_stage.h and csrc/td_sim_layout.h under the host compiler's address and undefined-behaviour
sanitizers: tests/stage_host_main.cpp is compiled as a stand-alone program and run as a child process.  No GPU, nothing is
loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_and_offset_check_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stage_host_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "taxidispatcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "stage_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-4000:] + r.stderr[-4000:]
