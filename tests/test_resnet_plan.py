"""The encoder's launch plan (st_resnet_plan, host-only): which kernel takes which layer and how BatchNorm statistics replicas flow.

tests/golden/resnet_plans.txt holds the launch list of one forward per configuration, as the engine logged it on a GPU
(ST_LAYER_LOG); the planner must reproduce it line for line.  `python tests/test_resnet_plan.py` rewrites the fixture from
st_resnet_plan -- for an intended route change only."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests._util import GOLDEN  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "resnet_plans.txt")


def _sections():
    """[(header, (version, dtype, H, W, B, train), [lines])] of the fixture; header lines read '== R101 bf16 224x224 B=128 train'."""
    out = []
    for line in open(FIXTURE):
        line = line.rstrip("\n")
        if line.startswith("== "):
            v, dt, hw, b, mode = line[3:].split()
            h, w = hw.split("x")
            out.append((line, (int(v[1:]), dt, int(h), int(w), int(b[2:]), mode == "train"), []))
        elif line and not line.startswith("#"):
            out[-1][2].append(line)
    return out


_handles = {}


def _handle(version, dtype):
    from showtell_amd import _lib
    L = _lib.lib()
    key = (version, dtype)
    if key not in _handles:
        h = C.c_void_p()
        _lib.check(L.st_resnet_create(version, _lib.ST_BF16 if dtype == "bf16" else _lib.ST_F32, C.byref(h)), "st_resnet_create")
        _handles[key] = h
    return L, _handles[key]


def plan_refusal(version, dtype, H, W, B, train):
    """(st_resnet_plan's return value, st_last_error's text) for arguments the planner is expected to refuse"""
    L, h = _handle(version, dtype)
    n = L.st_resnet_plan(h, B, H, W, int(train), None, 0)
    return n, L.st_last_error().decode()


def plan(version, dtype, H, W, B, train):
    L, h = _handle(version, dtype)
    n = L.st_resnet_plan(h, B, H, W, int(train), None, 0)
    assert n > 0, L.st_last_error()
    buf = C.create_string_buffer(n + 1)
    assert L.st_resnet_plan(h, B, H, W, int(train), buf, n + 1) == n
    return buf.value.decode().splitlines()


def fields(line):
    f = line.split(",")
    return dict(family=f[0], cin=int(f[2]), cout=int(f[3]), k=int(f[4]), stride=int(f[5]), rep_out=int(f[10]), rep_in=int(f[11]))


SECTIONS = _sections()


@pytest.mark.parametrize("cfg,lines", [(s[1], s[2]) for s in SECTIONS], ids=[s[0][3:].replace(" ", "_") for s in SECTIONS])
def test_plan_matches_the_logged_launches(cfg, lines):
    got = plan(*cfg)
    assert len(got) == len(lines)
    for i, (g, e) in enumerate(zip(got, lines)):
        assert g == e, "launch %d" % i


@pytest.mark.parametrize("cfg", [s[1] for s in SECTIONS] + [(101, "bf16", 448, 448, 668, True), (101, "bf16", 448, 448, 669, True)])
def test_igemm_reads_reduced_statistics(cfg):
    """st_conv's input transform reads replica 0 only: whatever feeds it BatchNorm statistics has them reduced first."""
    for line in plan(*cfg):
        f = fields(line)
        if f["family"] == "igemm":
            assert f["rep_in"] <= 1, line


def _layer2_conv2(lines):
    i = next(i for i, line in enumerate(lines) if fields(line)["k"] == 3 and fields(line)["stride"] == 2 and fields(line)["cin"] == 128)
    return i, fields(lines[i])


def test_stride2_conv_falls_back_behind_a_reduction_past_the_2_31_guard():
    # B = 668 at 448 x 448: the stride-2 kernel takes layer2's first conv2 and sums conv1's four replicas itself
    lines = plan(101, "bf16", 448, 448, 668, True)
    _, f = _layer2_conv2(lines)
    assert (f["family"], f["rep_in"]) == ("conv3x3_s2", 4)
    # B = 669: B * 112 * 112 * 128 * 2 >= 2^31, the conv runs on st_conv, which reads replica 0 -- conv1's replicas are reduced before it
    lines = plan(101, "bf16", 448, 448, 669, True)
    i, f = _layer2_conv2(lines)
    assert (f["family"], f["rep_in"]) == ("igemm", 1)
    red = fields(lines[i - 1])
    assert (red["family"], red["cout"], red["rep_out"], red["rep_in"]) == ("bn_reduce_replicas", 128, 1, 4)


if __name__ == "__main__":
    head = [line for line in open(FIXTURE) if line.startswith("#")]
    with open(FIXTURE, "w") as f:
        f.writelines(head)
        for header, cfg, _ in SECTIONS:
            f.write(header + "\n")
            f.writelines(line + "\n" for line in plan(*cfg))
    print("rewrote", FIXTURE)
