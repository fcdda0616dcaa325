"""Builds a lock-step host emulator of one gather-kernel file (tests/kernel_emu/): the kernel source and csrc/row_tiles.hpp are
compiled UNMODIFIED with g++ against host stand-ins for common.hpp and edge_args.hpp, next to the runtime (fibers, guarded buffers)
and the kernel's own main."""
import os
import shutil
import subprocess

from conftest import ROOT


def build_emulator(tmp_path_factory, kernel, main):
    """kernel: a file of dgll_amd/csrc, main: a file of tests/kernel_emu -> path of the executable"""
    work = tmp_path_factory.mktemp(kernel.replace(".", "_") + "_emu")
    for name in ("common.hpp", "edge_args.hpp", "emu_runtime.hpp", main):
        shutil.copy(os.path.join(ROOT, "tests", "kernel_emu", name), work)
    for name in ("row_tiles.hpp", kernel):
        shutil.copy(os.path.join(ROOT, "dgll_amd", "csrc", name), work)
    exe = str(work / "emu")
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-x", "c++", str(work / main), "-I", os.path.join(ROOT, "include"),
                    "-o", exe], check=True, capture_output=True, text=True)
    return exe
