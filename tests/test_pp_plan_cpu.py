"""chomp_pp_plan.h without a GPU: tests/hostcheck/ppcheck.cpp, the planner of the projection sets'
arena of tabulated redshift distributions, built with the address and undefined-behaviour
sanitizers and run as a program of its own."""
import os
import subprocess

from conftest import ROOT


def test_ppcheck_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ppcheck")
    src = os.path.join(ROOT, "tests", "hostcheck", "ppcheck.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "ppcheck ok" in run.stdout
