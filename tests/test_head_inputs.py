"""The inputs of tests/test_gpu_head.py have power: from the hand-written oracle alone (nothing of showtell_amd is used), every
case reaches the branch its row names, the float32 replica (in bf16 mode: the float64 replica that rounds dz to bf16) stays
inside the bounds that the GPU test holds the kernels to, and the replica with any one seeded fault falls outside them.
Nothing here needs a GPU."""
import pytest
import torch

from tests import _head_cases as H

# B, F, E; then per dtype (fp32, bf16) whether the forward GEMM runs split-K
TABLE = {
    "tiny": (3, 8, 4, False, False),
    "odd": (13, 64, 36, False, False),
    "single": (1, 512, 256, True, True),
    "split_edge": (70, 512, 100, True, True),
    "long_k": (9, 1000, 64, False, False),
    "tall": (257, 256, 32, True, False),
}


def test_the_cases_are_what_the_table_says():
    assert list(H.CASES) == list(TABLE)
    for case, (B, F, E, split32, split16) in TABLE.items():
        assert H.CASES[case][:3] == (B, F, E)
        assert H.CASES[case][3] == (("eval",) if case == "single" else ("train", "eval"))
        assert F % 8 == 0 and E % 4 == 0                                  # what st_linear_bn1d_forward accepts
        for dtype, want in zip(H.DTYPES, (split32, split16)):
            bk = {"float32": 32, "bfloat16": 64}[dtype]
            assert H.split_k(B, F, E, dtype) == (F % (8 * bk) == 0 and B * E <= 256 * 128 * 64) == want, (case, dtype)
    Bp = {c: H.up8(v[0]) for c, v in TABLE.items()}
    Ep = {c: H.up8(v[2]) for c, v in TABLE.items()}
    assert Bp == {"tiny": 8, "odd": 16, "single": 8, "split_edge": 72, "long_k": 16, "tall": 264}
    assert Ep == {"tiny": 8, "odd": 40, "single": 256, "split_edge": 104, "long_k": 64, "tall": 32}
    assert {c: v[2] % 32 for c, v in TABLE.items()} == {"tiny": 4, "odd": 4, "single": 0, "split_edge": 4, "long_k": 0, "tall": 0}
    assert TABLE["odd"][0] % 8 == 5 and TABLE["long_k"][1] % 256 != 0 and TABLE["long_k"][1] > 512
    assert (TABLE["split_edge"][0] + 63) // 64 == 2 and (TABLE["tall"][0] + 63) // 64 == 5 and (TABLE["tall"][0] + 7) // 8 == 33
    assert all(c in H.CASES and "train" in H.CASES[c][3] for c in H.ACCUMULATION_CASES)
    # the workspace: three 256-aligned regions
    assert H.workspace_bytes(3, 8, 4, "float32") == 256 + 256 + 256 and H.workspace_bytes(3, 8, 4, "bfloat16") == 768
    assert H.workspace_bytes(70, 512, 100, "bfloat16") == H.al256(70 * 104 * 2) + H.al256(100 * 72 * 2) + H.al256(512 * 72 * 2)


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_the_inputs_are_drawn_as_the_cases_file_says(dtype):
    for case, (B, F, E, _) in H.CASES.items():
        p = H.inputs(case, dtype)
        assert p["x"].shape == p["x2"].shape == (B, F) and p["W"].shape == p["g0_dW"].shape == (E, F) and p["dy"].shape == p["dy2"].shape == (B, E)
        assert all(p[k].shape == (E,) for k in ("b", "gamma", "beta", "running_mean", "running_var", "g0_dbias", "g0_dgamma", "g0_dbeta"))
        assert all(v.dtype == torch.float32 for v in p.values())
        assert (p["x"] >= 0).all() and (p["x2"] >= 0).all() and not torch.equal(p["x"], p["x2"])
        assert p["b"].abs().max() <= F ** -0.5 and 0.5 <= p["gamma"].min() and p["gamma"].max() < 1.5
        assert 0.5 <= p["running_var"].min() and p["running_var"].max() < 1.5
        assert all(p["g0_" + k].abs().min() > 0 for k in H.GRADS)               # a start that accumulation cannot hide behind
        if F * E >= 4096:
            assert abs(p["W"].std().item() / 0.05 - 1) < 0.05
        for k in ("x", "x2", "W"):
            assert torch.equal(p[k].bfloat16().float(), p[k]) == (dtype == "bfloat16")
    if dtype == "float32":
        z = H.oracle(H.inputs("tiny", dtype), H.inputs("tiny", dtype)["x"], H.inputs("tiny", dtype)["dy"], torch.zeros(4), torch.ones(4), True)
        assert torch.isfinite(z["dW"]).all() and z["dbias"].abs().max() < 1e-12                 # train: dbias is analytically zero


def _runs():
    for case, (B, F, E, modes) in H.CASES.items():
        for mode in modes:
            for steps in (1, 2) if case in H.ACCUMULATION_CASES else (1,):
                yield case, mode == "train", steps


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_the_replica_is_inside_the_bounds(dtype):
    worst = {}
    for case, train, steps in _runs():
        ref = H.run(case, dtype, train, steps=steps)
        assert all(torch.isfinite(v).all() for v in ref.values())
        if dtype == "float32":
            got = H.run(case, dtype, train, torch.float32, steps=steps)
        else:
            got = H.run(case, dtype, train, round_dz=True, steps=steps)
        errs = H.errors(got, ref, train)
        assert set(errs) == set(H.TENSORS)
        print(f"MEASURE {dtype} replica {case} {'train' if train else 'eval'} steps={steps}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert not H.outside(errs, dtype), (case, train, steps, errs)
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"MEASURE {dtype} replica, worst per tensor: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # the bounds are what the cases file says they are: 10 x and 4 x the replica's largest error, to two digits
    if dtype == "float32":
        assert 0.95 * H.BOUND_F32 <= 10 * max(worst.values()) <= 1.05 * H.BOUND_F32
    else:
        assert 0.95 * H.BOUND_BF16_DZ <= 4 * worst["dW"] <= 1.05 * H.BOUND_BF16_DZ and worst["dbias"] <= worst["dW"]


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("fault", list(H.FAULTS))
def test_every_seeded_fault_is_outside_the_bounds(fault, dtype):
    """In every case whose table row names the fault's branch, and in every mode the fault applies to."""
    replicas = (torch.float64, torch.float32) if dtype == "float32" else (torch.float64,)
    shown = 0
    for case, (B, F, E, modes) in H.CASES.items():
        for mode in modes:
            train = mode == "train"
            if not H.FAULTS[fault](B, F, E, dtype, train):
                continue
            ref = H.run(case, dtype, train)
            for rep in replicas:
                errs = H.errors(H.run(case, dtype, train, rep, dtype == "bfloat16", fault), ref, train)
                out = H.outside(errs, dtype)
                listed = case in H.fault_cases(fault)
                print(f"MEASURE {dtype} fault {fault} {case} {mode} ({str(rep)[6:]}){'' if listed else ' [not required]'}: "
                      + (" ".join(f"{k} {errs[k]:.1e}" for k in out) or "inside"))
                if listed:
                    assert out, (fault, dtype, case, mode, errs)
                    shown += 1
    assert shown, f"no case of {fault} applies in {dtype}"


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("case", H.ACCUMULATION_CASES)
def test_overwriting_instead_of_accumulating_is_outside_the_bounds(case, dtype):
    for train in (True, False):
        ref = H.run(case, dtype, train, steps=2)
        one = H.run(case, dtype, train, steps=1)
        assert all(not torch.equal(ref[k], one[k]) for k in ("dW", "dgamma", "dbeta"))       # the second call adds something
        errs = H.errors(H.run(case, dtype, train, torch.float64, dtype == "bfloat16", H.ACCUMULATION_FAULT, steps=2), ref, train)
        print(f"MEASURE {dtype} fault {H.ACCUMULATION_FAULT} {case} {'train' if train else 'eval'}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        # every one of the four shows it, but for the train-mode dbias in bf16: a lost g0 of about 1 is measured there against
        # the 2 B terms |dz| that cancel in it, and B = 70 rows of them hide it under the bf16 bound; eval mode shows that path
        for k in H.GRADS:
            if not (k == "dbias" and train and dtype == "bfloat16"):
                assert k in H.outside(errs, dtype), (k, errs)
