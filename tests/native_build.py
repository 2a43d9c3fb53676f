"""The g++ builds the CPU tests share: a stand-alone program of tests/native (its own main over tests/native/banded_walk.h),
a few extern "C" lines around qe_types.h as a shared object for ctypes, and the library's host layer linked with a driver
program (build_host).  All see the fake HIP runtime of tests/native/hip_stub, so the kernels' headers are plain C++.  Test
infrastructure only."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

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


HOST_SOURCES = ["qe_driver.hip", "qe_capi.cpp", "qe_hostpack.cpp"]
HOST_FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unused-parameter",
              "-Wno-class-memaccess", "-DQE_KERNELS_HEADER=\"qe_kernels_stub.h\"", "-I" + os.path.join(ROOT, "tests", "native", "hip_stub"),
              "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "quicked_amd", "csrc")]
ASAN_UBSAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
_host_objects = {}                 # sanitize flags -> the three objects, compiled once per process


def build_host(driver_cpp, out_dir, sanitize_flags):
    """The library's host layer (kernels = the stand-ins of hip_stub/qe_kernels_stub.h) + tests/native/<driver_cpp> under
    sanitize_flags -> the stand-alone executable in out_dir.  The library's sources are compiled once per flag set."""
    flags = HOST_FLAGS + list(sanitize_flags)
    key = tuple(sanitize_flags)
    if key not in _host_objects:
        obj_dir = tempfile.mkdtemp(prefix="qe_host_objects_")
        atexit.register(shutil.rmtree, obj_dir, ignore_errors=True)
        objs = [os.path.join(obj_dir, src.split(".")[0] + ".o") for src in HOST_SOURCES]
        procs = [subprocess.Popen(["g++"] + flags + ["-x", "c++", "-c", os.path.join(ROOT, "quicked_amd", "csrc", src), "-o", obj],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for src, obj in zip(HOST_SOURCES, objs)]
        for p in procs:
            err = p.communicate(timeout=900)[1]
            assert p.returncode == 0, err[-4000:]
        _host_objects[key] = objs
    exe = os.path.join(str(out_dir), os.path.splitext(driver_cpp)[0])
    built = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "native", driver_cpp)] + _host_objects[key] + ["-o", exe],
                           capture_output=True, text=True, timeout=900)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe
