"""Builds and loads tests/hostcheck/libhostcheck.so: chomp_math.h compiled for the host, the
serial counterpart the device harnesses and the CPU tests compare with.  Rebuilt when the source
or the header is newer than the library."""
import ctypes
import os
import subprocess

from conftest import ROOT

HC = os.path.join(ROOT, "tests", "hostcheck")


def load():
    so, src = os.path.join(HC, "libhostcheck.so"), os.path.join(HC, "hostcheck.cpp")
    hdr = os.path.join(ROOT, "chomp_amd", "csrc", "chomp_math.h")
    if (not os.path.exists(so) or
            os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)
