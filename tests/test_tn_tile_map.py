"""The LDS index arithmetic of the token-contraction GEMM (csrc/tn_tile.h) on the CPU.

tests/tn_tile_map.cpp is built with the host compiler and -fsanitize=address,undefined as a program of its own and run once.
It emulates an LDS image and the documented semantics of ds_read_b64_tr_b16 and checks, for the one tile shape gemm_tn_kernel
instantiates (32 rows x 128 columns per image), that every lane of every 16x16x32 operand fragment receives the element its
operand map requires, that every lane address is 8-byte aligned and inside the image, and counts the bank conflicts of the
transposed reads and of the loader's 16-byte stores.  DESIGN.md (4d, the token contraction) states 0 for both; the same reads
on 256-byte rows without the chunk XOR put the eight rows of a half-wave on the same banks (8-way: 7 extra cycles in each of the
32 half-wave reads = 224), which is the check that the counter counts.

Also here, because tests/test_abi.py fixes the set of structs _lib.py mirrors: the layout of gemm_tn.GemmTnDesc against the header.
"""
import functools
import os
import re
import subprocess
import tempfile

from tests._util import ROOT
from tests.test_abi import layout_errors

CSRC = os.path.join(ROOT, "show-tell_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _report():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "tn_tile_map")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, os.path.join(ROOT, "tests", "tn_tile_map.cpp"), "-o", exe])
        run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    return run


def test_every_lane_gets_the_element_the_operand_map_requires():
    run = _report()
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "FAIL" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_bank_conflicts_are_what_design_states():
    m = re.search(r"tile 32x128 read_conflicts=(\d+) write_conflicts=(\d+) plain_read_conflicts=(\d+)", _report().stdout)
    assert m, _report().stdout
    rd, wr, plain = map(int, m.groups())
    print(f"MEASURE transposed reads {rd} extra cycles, stores {wr}, reads without the XOR {plain}")
    assert rd == 0 and wr == 0
    assert plain == 224


def test_gemm_tn_desc_has_the_headers_layout():
    from showtell_amd.gemm_tn import GemmTnDesc
    assert layout_errors([(GemmTnDesc, "st_gemm_tn_desc")]) == []
