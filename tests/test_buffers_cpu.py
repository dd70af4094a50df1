"""chomp_buffers.h without a GPU: tests/hostcheck/bufcheck.cpp, the owning buffer types over
counting stand-ins for the allocation calls, built with the address and undefined-behaviour
sanitizers and run as a program of its own."""
import os
import subprocess

from conftest import ROOT


def test_bufcheck_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bufcheck")
    src = os.path.join(ROOT, "tests", "hostcheck", "bufcheck.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "bufcheck ok" in run.stdout
