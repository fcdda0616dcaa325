"""Builds a lock-step host emulator of one gather-kernel file (tests/kernel_emu/): the kernel source and csrc/row_tiles.hpp are
compiled UNMODIFIED with g++ against host stand-ins for common.hpp and edge_args.hpp, next to the runtime (fibers, guarded buffers)
and the kernel's own main."""
import os
import shutil
import subprocess

from conftest import ROOT


def rocm_clang():
    """The ROCm clang++, used as a plain host compiler (no offload) for a kernel file whose ext_vector_type typedefs g++ rejects."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for path in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(path):
            return path
    raise RuntimeError("no clang++ under %s" % rocm)


def build_emulator(tmp_path_factory, kernel, main, compiler=None):
    """kernel: a file of dgll_amd/csrc, main: a file of tests/kernel_emu -> path of the executable (compiler: g++ when None)"""
    work = tmp_path_factory.mktemp(kernel.replace(".", "_") + "_emu")
    for name in ("common.hpp", "edge_args.hpp", "emu_runtime.hpp", main):
        shutil.copy(os.path.join(ROOT, "tests", "kernel_emu", name), work)
    for name in ("row_tiles.hpp", kernel):
        shutil.copy(os.path.join(ROOT, "dgll_amd", "csrc", name), work)
    exe = str(work / "emu")
    subprocess.run([compiler or shutil.which("g++") or "g++", "-O1", "-std=c++17", "-x", "c++", str(work / main), "-I", os.path.join(ROOT, "include"),
                    "-o", exe], check=True, capture_output=True, text=True)
    return exe
