"""What the tests of the C++ host programs (tests/cpp) share: the one compile-and-link command, and the Python side of
the bit-level checksum the programs print (tests/cpp/app_util.hpp)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# extra flags of a program that includes the HIP runtime API itself (rod_dist_app)
HIP_HOST_FLAGS = ("-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include")


def compile_cpp(src, exe, extra=()):
    """src -> exe against include/ and the built library (warnings are errors); extra: further compiler flags"""
    from mundy_amd import build
    libdir = os.path.dirname(build.build())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra, str(src),
                           "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lmundy_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", str(exe)])
    return str(exe)


def build_app(name, extra=()):
    """tests/cpp/<name>.cpp -> tests/cpp/<name>; returns the executable's path"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    return compile_cpp(os.path.join(cpp, name + ".cpp"), os.path.join(cpp, name), extra)


def fnv1a(words):
    """order-sensitive FNV-1a over 64-bit words (an iterable of ints), as 16 hexadecimal digits"""
    h = 1469598103934665603
    for b in words:
        h = ((h ^ int(b)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def fnv1a_bits(a):
    """fnv1a over the bit patterns of an array of 8-byte items"""
    return fnv1a(np.ascontiguousarray(a).view(np.uint64).ravel().tolist())


def checksums(stdout):
    """the 'CHECKSUM name value [name value ...]' lines of a program's output as one dict of strings"""
    out = {}
    for ln in stdout.splitlines():
        if ln.startswith("CHECKSUM"):
            w = ln.split()
            out.update(zip(w[1::2], w[2::2]))
    return out
