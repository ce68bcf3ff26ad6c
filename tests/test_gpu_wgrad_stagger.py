"""The first-layer wgrad's f16x2 main loop (bf3_gemm_tn_rs_kernel<*, 1>, csrc/bf3_wgrad.hip) consumes and re-issues its operand loads
at three points of a k-tile: k-step 0 of x at the top, k-step 1 of x (and the next ids) inside the MFMA group loop, dy further down.
What that order can get wrong is a register set that is read before its load has landed or re-issued before it was read, and the
loads of k-tiles past a slice's end, which are now issued from inside the loop.  So the shapes here are the small ones: slices of
one, two and three k-tiles, a partial last k-tile, a last slice shorter than the others, f-tiles with waves that own no column, the
dense-feature wave, a second f-tile; ids with missing entries, repeated rows and a field that is missing altogether.

* dr_h2_wgrad_emb (both parts) and dr_h2_wgrad against x^T dy and sum(dy) in float64, at the tolerance tests/test_gpu_h2_gemm.py
  applies to this kernel: within 3e-6 of the largest output and no worse than 1.5 x the bf16x3 mode's error (+ 1e-7); the column sums
  bit-identical to the bf16x3 mode's (both add the unscaled fp32 values in one order).
* The gather form and the dense form on the materialised x with the same records: the same template and the same order of
  operations, so dstW and dstb must be bit-identical.
* DeepFMEngine: one plain and three prefetched train_steps at B = 2304, F = 3, V = 1000, DNN [256, 32] against the float64 step
  oracle of tests/engine_oracle.py, at that file's tolerances.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine_oracle as EO
from oracle import tf_semantics as O
from oracle import torch_ref as T

D, V = 64, 97


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _rel(got, ref):
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _inputs(R, F, N):
    """table, row_base, ids [R, nf] (10 % missing, every 5th example a copy of example 0, the last of several fields all missing),
    dense_pad (None without dense features), dy, and x = concat(gathered rows, dense features) as the gather form reads it."""
    nf, Nd = F // D, F % D
    g = torch.Generator(device="cuda").manual_seed(1000 * R + F + N)
    table = torch.randn((nf * V, D), device="cuda", generator=g) * 0.3
    row_base = (torch.arange(nf, device="cuda") * V).to(torch.int64)
    ids = torch.randint(0, V, (R, nf), device="cuda", generator=g)
    ids[torch.rand((R, nf), device="cuda", generator=g) < 0.1] = -1
    ids[5::5] = ids[0]
    if nf > 1:
        ids[:, nf - 1] = -1
    dpad = None
    if Nd:
        dpad = torch.zeros((R, 32), device="cuda")
        dpad[:, :Nd] = torch.randn((R, Nd), device="cuda", generator=g) * 15
    dy = torch.randn((R, N), device="cuda", generator=g) * 1e-3
    return table, row_base, ids, dpad, dy


def _materialise(table, row_base, ids, dpad, F):
    R, nf = ids.shape
    x = torch.zeros((R, (F + 3) // 4 * 4), device="cuda")
    rows = table[(row_base[None, :] + ids.clamp_min(0)).reshape(-1)].view(R, nf, D)
    x[:, :nf * D] = (rows * (ids >= 0)[:, :, None]).reshape(R, nf * D)
    if dpad is not None:
        x[:, nf * D:F] = dpad[:, :F - nf * D]
    return x[:, :F]


def _nan_ws(ops, R, F, N):
    return ops.bf3_wgrad_workspace(R, F, N, "cuda").fill_(float("nan"))


def _check_gather(ops, table, row_base, ids, dpad, dy, F, what):
    """Both modes' gathering wgrad against float64; returns the f16x2 results, the records and x."""
    R, N = dy.shape
    x = _materialise(table, row_base, ids, dpad, F)
    ref, refb = x.double().t() @ dy.double(), dy.double().sum(0)
    ids_t = ids.t().contiguous().to(torch.int32)
    tam, dam, dyam = ops.h2_amax(table), ops.h2_amax(dpad) if dpad is not None else None, ops.h2_amax(dy)
    d3, d2 = torch.zeros((F, N), device="cuda"), torch.zeros((F, N), device="cuda")
    b3, b2 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    ops.bf3_wgrad_emb(ids_t, row_base, table, dpad, dy, 1.0, d3, b3)
    ops.h2_wgrad_emb(ids_t, row_base, table, tam, dpad, dam, dy, dyam, 1.0, d2, b2, workspace=_nan_ws(ops, R, F, N), parts=3)
    e2, e3, eb = _rel(d2, ref), _rel(d3, ref), _rel(b2, refb)
    print("%s: x^T dy f16x2 %.3e bf16x3 %.3e of the largest output (bound 3e-6), sum(dy) %.3e" % (what, e2, e3, eb))
    assert e2 <= 3e-6 and e2 <= 1.5 * e3 + 1e-7, (what, e2, e3)
    assert eb <= 3e-6, (what, eb)
    assert torch.equal(b2, b3), what
    return x, d2, b2, (tam, dam, dyam)


@pytest.mark.parametrize("N", [32, 256])
@pytest.mark.parametrize("F", [64 * 1 + 13, 64 * 3, 64 * 5 + 13])
@pytest.mark.parametrize("R", [32, 40, 64, 96, 545, 1056 + 7])
def test_wgrad_gather_and_dense_forms_against_float64_and_each_other(ops, R, F, N):
    table, row_base, ids, dpad, dy = _inputs(R, F, N)
    x, d2, b2, (tam, dam, dyam) = _check_gather(ops, table, row_base, ids, dpad, dy, F, "R %d F %d N %d" % (R, F, N))
    # the dense form on the materialised x, with the record the gather form uses for x (the larger of the table's and the features')
    xam = torch.maximum(tam, dam) if dam is not None else tam.clone()
    dd, bd = torch.zeros((F, N), device="cuda"), torch.zeros(N, device="cuda")
    ops.h2_wgrad(x, xam, dy, dyam, 1.0, dd, bd, workspace=_nan_ws(ops, R, F, N))
    assert torch.equal(dd.view(torch.int32), d2.view(torch.int32)), "gather and dense form differ in dstW"
    assert torch.equal(bd.view(torch.int32), b2.view(torch.int32)), "gather and dense form differ in dstb"
    if F // D == 1:
        # a single field cannot lose all its ids above without emptying the whole gather: here it does, on its own
        _check_gather(ops, table, row_base, torch.full_like(ids, -1), dpad, dy, F, "R %d F %d N %d, the field all missing" % (R, F, N))


def test_engine_prefetched_steps_match_the_float64_oracle():
    """B = 2304, F = 3, V = 1000, DNN [256, 32], SGD at lr 1.0 (tests/test_gpu_engine_matrix.py): the step whose first-layer wgrad is
    dr_h2_wgrad_emb (asserted), one plain step and three prefetched ones, each against one float64 oracle step from the device's state."""
    from deep_recommenders_amd.engine import DeepFMEngine
    F, Ve, Nd, B, lr, steps = 3, 1000, 3, 2304, 1.0, 4
    eng = DeepFMEngine(F, Ve, D, [256, 32], B, num_dense=Nd, lr=lr, seed=42, hashed=True, lin_init_std=0.1, optimizer="sgd")
    assert eng.h2 and eng.no_concat and eng.fuse_k3, "the engine does not run the gathering f16x2 wgrad at this shape"
    g = torch.Generator(device="cuda").manual_seed(4321)
    batches, ids_list = [], []
    for _ in range(steps):
        keys = torch.randint(0, 10**12, (B, F), device="cuda", generator=g)
        k = keys.cpu().numpy()
        ids_list.append(np.stack([O.hash_bucket_i64(k[:, f], Ve) for f in range(F)], axis=1))
        batches.append((keys, torch.rand((B, Nd), device="cuda", generator=g), (torch.rand(B, device="cuda", generator=g) < 0.3).float()))
    orc = EO._CompactOracle(eng, ids_list, "sgd", lr, dtype=torch.float64, all_rows=True)
    ratios = {}
    for i, (keys, dense, labels) in enumerate(batches):
        orc.resync_from(eng)
        before = (orc.table.float(), orc.lin.float(), orc.bias.float(), [w.float() for w in orc.Ws], [b.float() for b in orc.bs])
        nk, nd = (batches[i + 1][0], batches[i + 1][1]) if i + 1 < steps else (None, None)
        loss = float(eng.train_step(keys, dense, labels, next_keys=nk, next_dense=nd).item())
        assert eng._plan_prefetched == (i > 0), "the prefetched plan was not picked up"
        np.testing.assert_array_equal(eng.ids.cpu().numpy(), ids_list[i])
        want = orc.step(i, dense.cpu(), labels.cpu(), relu_masks=EO._device_relu_masks(eng))
        T.check_ties(orc.ties, max_frac=1e-5)
        assert abs(loss - want) <= 1e-5 * abs(want), (i, loss, want)
        EO._check_sgd_step(eng, orc, before, orc.touched(i), ratios)
    print("worst error / tolerance per parameter over %d steps: %s" % (steps, {k: round(v, 3) for k, v in ratios.items()}))
