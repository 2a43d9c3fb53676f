"""The two g++ builds the CPU tests of the score-only walk share: a stand-alone program of tests/native (its own main over
tests/native/banded_walk.h) and a few extern "C" lines around qe_types.h as a shared object for ctypes.  Both see the fake
HIP runtime of tests/native/hip_stub, so the kernels' headers are plain C++.  Test infrastructure only."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "tests", "native", "hip_stub"), "-I", os.path.join(ROOT, "quicked_amd", "csrc")]


def build_walk(program, out_dir, sanitize=False):
    """tests/native/<program>.cpp -> the executable; sanitize: under ASan + UBSan, as <program>_san"""
    exe = os.path.join(out_dir, program + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + INCLUDES +
                   [os.path.join(ROOT, "tests", "native", program + ".cpp"), "-o", exe], check=True)
    return exe


def host_lib(out_dir, name, source_text):
    """source_text (after the includes of the HIP stub and qe_types.h) compiled for the host -> lib<name>.so, loaded"""
    src = os.path.join(out_dir, name + ".cpp")
    lib = os.path.join(out_dir, "lib" + name + ".so")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "qe_types.h"\n' + source_text)
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared"] + INCLUDES + [src, "-o", lib], check=True)
    return ctypes.CDLL(lib)
