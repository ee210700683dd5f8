"""The inputs of tests/test_gpu_grad_clip.py have power: from the torch replica alone (nothing of showtell_amd.optim is used), the
float32 replica stays inside the bound that the GPU test holds the kernels to, and the replica with any one seeded fault falls
outside it.  Nothing here needs a GPU."""
import pytest
import torch

from tests import _grad_clip_cases as G


def test_the_inputs_are_what_the_cases_file_says():
    ps, gs = G.params(), G.grads()
    assert [p.numel() for p in ps] == [1, 3, 35, 2112, 1025]
    assert sum((p.numel() + 3) // 4 * 4 for p in ps) == 3184
    assert sorted({p.numel() % 4 for p in ps}) == [0, 1, 3] and ps[0].numel() < 4       # padding 0, 3, 1 and a tail shorter than a vector
    assert len(gs) == 6
    for k, step in enumerate(gs):
        for g, p in zip(step, ps):
            assert g.shape == p.shape and (g.numel() < 35 or ((g > 0).any() and (g < 0).any()))
            fin = g[torch.isfinite(g)].abs() / G.SCALES[k]
            assert fin.min() >= 0.5 * (1 - 1e-6) and fin.max() < 2.0 * (1 + 1e-6)
        bad = sum(int((~torch.isfinite(g)).sum()) for g in step)
        assert bad == (1 if k == G.NAN_STEP else 0)
    assert gs[G.NAN_STEP][2].view(-1)[G.INF_AT[1]] == float("inf") and ps[2].shape == (5, 7)
    n = G.norms()
    print("MEASURE norms", ["%.4g" % v for v in n])
    for got, want in zip(n, [74, float("inf"), 2236, 0.74, 74, 74]):
        assert got == want or abs(got / want - 1) < 0.05
    active = [v > G.MAX_NORM for v in n if v != float("inf")]
    assert sum(active) == 4 and len(active) == 5                                        # the clip acts on four steps, not on one


@pytest.mark.parametrize("kind", G.KINDS)
def test_float32_replica_is_inside_the_bound_and_every_seeded_fault_outside(kind):
    ref = G.replica(kind)
    assert torch.isfinite(ref).all()
    own = G.rel_err(G.replica(kind, torch.float32), ref)
    print(f"MEASURE {kind} float32 replica vs float64: {own:.3e} (bound {G.BOUND:.0e})")
    assert own <= G.BOUND
    for fault, kinds in G.FAULTS.items():
        if kind not in kinds:
            continue
        for dtype in (torch.float64, torch.float32):
            err = G.rel_err(G.replica(kind, dtype, fault), ref)
            print(f"MEASURE {kind} fault {fault} ({str(dtype)[6:]}): {err:.3e}  = {err / G.BOUND:.0f} x bound")
            assert err > G.BOUND, (kind, fault, err)


@pytest.mark.parametrize("kind", G.KINDS)
def test_world_2_replica_equals_world_1_and_the_norm_of_the_summed_gradient_is_caught(kind):
    """Data parallel: flat_grad holds the SUM over ranks and grad_scale = 1 / world; the clipped quantity is the norm of the
    average.  Averaging first changes nothing (a power of two); taking the norm of the sum does."""
    ref = G.replica(kind)
    assert G.rel_err(G.replica(kind, world=2), ref) <= 1e-12
    err = G.rel_err(G.replica(kind, fault="summed_norm", world=2), ref)
    print(f"MEASURE {kind} fault summed_norm, world 2: {err:.3e}  = {err / G.BOUND:.0f} x bound")
    assert err > G.BOUND


@pytest.mark.parametrize("kind", ["Adam", "AdamW"])
def test_past_the_grid_cap_the_float32_replica_is_inside_the_bound_and_the_faults_outside(kind):
    """The inputs of test_three_steps_past_the_grid_cap_match_the_float64_replica: 2048 * 1024 + 5 and 3 elements."""
    ps, gs = G.long_params(), G.long_grads()
    assert [p.numel() for p in ps] == [2048 * 1024 + 5, 3] and len(gs) == 3
    n = sum((p.numel() + 3) // 4 * 4 for p in ps)
    trip = 2048 * 256 * 4                                       # what one pass of the capped grid covers
    assert n == 2097164 and (n // 4 + 255) // 256 > 2048 and trip < ps[0].numel() < trip + 8 and ps[0].numel() % 4 == 1
    norms = [torch.sqrt(sum((t.double() ** 2).sum() for t in step)).item() for step in gs]
    print("MEASURE long norms", ["%.4g" % v for v in norms])
    assert [v > G.MAX_NORM for v in norms] == [True, True, False]
    ref = G.replica(kind, long=True)
    assert torch.isfinite(ref).all() and ref.numel() == 2048 * 1024 + 8
    own = G.rel_err(G.replica(kind, torch.float32, long=True), ref)
    print(f"MEASURE {kind} long float32 replica vs float64: {own:.3e} (bound {G.BOUND:.0e})")
    assert own <= G.BOUND
    for fault in ("no_clip", "per_tensor_norm", "no_decay", "decay_swapped"):
        err = G.rel_err(G.replica(kind, fault=fault, long=True), ref)
        print(f"MEASURE {kind} long fault {fault}: {err:.3e}  = {err / G.BOUND:.0f} x bound")
        assert err > G.BOUND, (kind, fault, err)
