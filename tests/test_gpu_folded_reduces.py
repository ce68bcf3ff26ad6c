"""The first-layer wgrad's split-K reduce as rider blocks of a launch that is on the training stream anyway:
dr_emb_pool_bwd_dups_apply is K4's duplicate pass with the wgrad's reduce + SGD step (part 2 of dr_h2_wgrad_emb) riding in it.
The riders run the device function the stand-alone reduce kernel runs (csrc/tn_rs_reduce.h) on the same partials in the same order,
so every result must be BIT-identical to the unfolded calls -- compared as int32 views, at the kernels and over whole DeepFMEngine
steps.  The reduce takes its f16x2 scales from the amax words the main kernel saved in the workspace: the "scale trap" raises the
table's live record across a power of two between the two launches (what K4 does in a real step) and the bits must not move.
The CPU test holds the workspace accounting and the argument checks, which return before any launch.

(The tower tail's reduce riding in the wgrad's main launch was built as well, was bit-identical at M = 544 and M = 32, did not pay on
the GPU and was removed with its entry point: DESIGN.md 3.5.)"""
import ctypes

import numpy as np
import pytest
import torch

D, V = 64, 1000
LR = 0.05


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the wgrad's reduce in the duplicate pass's launch ------------------------------------------------------------------------------------
def _wgrad_scene():
    """R = 2048 + 96 rows: split >= 2, the last slice ends in a partial k-tile.  3 fields + 13 dense columns: in_dim 205, one ragged f-tile."""
    R, F, nd, N = 2048 + 96, 3, 13, 256
    g = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, V, size=(R, F))
    ids[rng.random((R, F)) < 0.05] = -1
    ids = torch.as_tensor(ids).cuda()
    s = dict(R=R, F=F, nd=nd, N=N, K=F * D + nd, ids=ids, row_base=(torch.arange(F, dtype=torch.int64) * V).cuda())
    s["table"] = torch.randn((F * V, D), device="cuda", generator=g) * 0.125
    s["lin"] = torch.randn(F * V, device="cuda", generator=g) * 0.01
    s["dense"] = torch.zeros((R, 32), device="cuda")
    s["dense"][:, :nd] = torch.rand((R, nd), device="cuda", generator=g)
    s["dy"] = torch.randn((R, N), device="cuda", generator=g) * (torch.rand((R, N), device="cuda", generator=g) > 0.5) / R
    s["W0"] = torch.randn((s["K"], N), device="cuda", generator=g) / s["K"] ** 0.5
    s["b0"] = torch.randn(N, device="cuda", generator=g) * 0.1
    s["dl"] = torch.randn(R, device="cuda", generator=g) / R
    s["d_concat"] = torch.randn((R, (s["K"] + 3) // 4 * 4), device="cuda", generator=g) / R
    idc = ids.clamp_min(0) + s["row_base"][None, :]
    s["sum_x"] = (s["table"][idc] * (ids >= 0)[..., None]).sum(1).contiguous()
    s["lin_old_t"] = s["lin"][idc].t().contiguous()
    return s


def _wgrad_then_dups(ops, s, folded, trap=False):
    """wgrad of the first layer, then K4's duplicate pass (parts 1 | 8 and 2 | 8).  Returns W0, b0, table, lin_w, lin_bias and the table's record."""
    R, F, N = s["R"], s["F"], s["N"]
    W0, b0 = s["W0"].clone(), s["b0"].clone()
    table, lin, bias = s["table"].clone(), s["lin"].clone(), torch.zeros(1, device="cuda")
    plan = ops.emb_sort_slots(s["ids"], s["row_base"], F * V)
    ids_t = ops.ids_transpose_i32(s["ids"])
    tab_am, den_am, dy_am = ops.h2_amax(table), ops.h2_amax(s["dense"]), ops.h2_amax(s["dy"])
    ws = ops.bf3_wgrad_workspace(R, s["K"], N, "cuda").fill_(float("nan"))
    xs = torch.full((R * F, D), float("nan"), device="cuda")

    def raise_record():
        if trap:                                     # the record K4 keeps: two powers of two up, written directly
            tab_am.copy_((tab_am.view(torch.float32) * 4.0).view(torch.int32))

    if folded:
        ops.h2_wgrad_emb(ids_t, s["row_base"], table, tab_am, s["dense"], den_am, s["dy"], dy_am, -LR, W0, b0, workspace=ws, parts=1)
        assert torch.equal(W0, s["W0"]) and torch.equal(b0, s["b0"])          # (part 1 leaves the layer alone)
        raise_record()
        ops.emb_pool_bwd_dups_apply(s["ids"], s["row_base"], plan, D, F * V, s["d_concat"], s["dl"], -LR, table, lin, bias, s["sum_x"], xs,
                                    s["lin_old_t"], tab_am, ws, R, -LR, W0, b0, wg_h2=True, parts=1)
    else:
        ops.h2_wgrad_emb(ids_t, s["row_base"], table, tab_am, s["dense"], den_am, s["dy"], dy_am, -LR, W0, b0, workspace=ws, parts=3)
        raise_record()
        ops.emb_pool_bwd_sorted(s["ids"], s["row_base"], plan, D, F * V, s["d_concat"], s["dl"], -LR, table, lin, bias, sum_x=s["sum_x"],
                                x_sorted=xs, parts=1 | 8, lin_old_t=s["lin_old_t"], table_amax=tab_am)
    ops.emb_pool_bwd_sorted(s["ids"], s["row_base"], plan, D, F * V, s["d_concat"], s["dl"], -LR, table, lin, bias, sum_x=s["sum_x"],
                            x_sorted=xs, parts=2 | 8, lin_old_t=s["lin_old_t"], table_amax=tab_am)
    torch.cuda.synchronize()
    return dict(W0=W0, b0=b0, table=table, lin=lin, bias=bias, rec=tab_am.clone())


@pytest.fixture(scope="module")
def wgrad_runs(ops):
    s = _wgrad_scene()
    return s, _wgrad_then_dups(ops, s, False), _wgrad_then_dups(ops, s, True), _wgrad_then_dups(ops, s, True, trap=True)


@pytest.mark.gpu
def test_wgrad_riders_in_the_dups_launch_give_the_reduce_kernels_bits(wgrad_runs):
    s, ref, new, _ = wgrad_runs
    assert not torch.equal(ref["W0"], s["W0"]) and not torch.equal(ref["b0"], s["b0"])        # the step did move the layer
    assert bool(torch.isfinite(new["W0"]).all())
    for k in ("W0", "b0", "table", "lin", "bias", "rec"):
        assert torch.equal(_bits(new[k]), _bits(ref[k])), k
    assert not torch.equal(ref["table"], s["table"])                                          # ... and the duplicate pass the table


@pytest.mark.gpu
def test_scale_trap_the_deferred_reduce_does_not_read_the_live_record(wgrad_runs):
    s, ref, _, trapped = wgrad_runs
    assert torch.equal(_bits(trapped["W0"]), _bits(ref["W0"])), "W0 moved with the table's record: %d elements" % int(
        (trapped["W0"] != ref["W0"]).sum().item())
    assert torch.equal(_bits(trapped["b0"]), _bits(ref["b0"]))
    assert int(trapped["rec"].item()) > int(ref["rec"].item())                                    # the trap was set


# ---- whole steps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [50, 100000])   # duplicates and hot rows in every step; nearly all rows unique
def test_engine_steps_are_bit_identical_with_the_reduces_folded(vocab, monkeypatch):
    from deep_recommenders_amd.engine import DeepFMEngine
    B, F, Nd = 2048, 3, 13
    g = torch.Generator(device="cuda").manual_seed(vocab)
    batches = [(torch.randint(0, 10**12, (B, F), device="cuda", generator=g), torch.rand((B, Nd), device="cuda", generator=g),
                (torch.rand(B, device="cuda", generator=g) < 0.3).float()) for _ in range(2)]

    def run():
        eng = DeepFMEngine(F, vocab, D, [256, 32], B, num_dense=Nd, lr=LR, seed=3, lin_init_std=0.1)
        snaps = []

        def snap():
            torch.cuda.synchronize()
            snaps.append([t.clone() for t in (eng.table, eng.lin_w, eng.flat_params, eng.prob, eng.loss)])
        for n in range(4):                            # four prefetched steps over two alternating batches
            k, d, l = batches[n % 2]
            nk, nd = batches[(n + 1) % 2][:2]
            eng.train_step(k, d, l, next_keys=nk, next_dense=nd)
            snap()
        eng.Ws[0].mul_(0.5)                           # an outside write: the forward re-splits W0, the step's refresh follows the apply
        k, d, l = batches[0]
        eng.train_step(k, d, l)
        snap()
        eng.train_step(*batches[1])                   # ... and this forward reads the planes that refresh made
        snap()
        return eng, snaps
    on, s_on = run()
    assert on.fold_reduces and on.tail_in_fwd and on.fuse_k4
    monkeypatch.setenv("DR_FOLD_REDUCES", "0")
    off, s_off = run()
    assert not off.fold_reduces and off.tail_in_fwd and off.fuse_k4
    for n, (a, b) in enumerate(zip(s_on, s_off)):
        for x, y, what in zip(a, b, ("table", "lin_w", "flat_params", "prob", "loss")):
            assert torch.equal(_bits(x), _bits(y)), "step %d: %s" % (n, what)
    assert not torch.equal(s_on[0][2], s_on[1][2])    # the dense parameters do move from step to step


# ---- no GPU: workspace accounting and argument checks --------------------------------------------------------------------------------------
def test_workspace_header_and_refusals_before_any_launch():
    from deep_recommenders_amd import _lib
    L = _lib.lib()
    R, K, N = 2048 + 96, 205, 256
    # tn_rs_plan: one f-tile, one n-tile, at least 16 k-tiles per slice -> 5 slices; [split][256][256] + [split][256] + a 16-byte header
    split = 5
    assert L.dr_bf3_wgrad_workspace_bytes(R, K, N) == 4 * (split * 256 * 256 + split * 256) + 16
    assert L.dr_bf3_wgrad_workspace_bytes(65536, 1677, 256) == 4 * (36 * 1792 * 256 + 36 * 256) + 16
    assert L.dr_bf3_wgrad_workspace_bytes(0, K, N) == 0
    need = L.dr_bf3_wgrad_workspace_bytes(R, K, N)
    buf = (ctypes.c_char * 64)()                      # something that is not NULL; a refused call touches none of it
    p = ctypes.addressof(buf)

    def dups_apply(ws, ws_bytes):
        return L.dr_emb_pool_bwd_dups_apply(p, p, p, p, p, p, p, R, 3, 64, 3000, p, 208, p, p, -0.05, p, p, p, p, p, 1 | 8, p, ws, ws_bytes,
                                            R, K, N, 1, -0.05, p, N, p, None)
    assert dups_apply(None, need) == _lib.DR_EINVAL
    assert dups_apply(p, need - 4) == _lib.DR_EINVAL
    assert dups_apply(p, need - 16) == _lib.DR_EINVAL                 # the size before the header existed
    assert bytes(buf) == bytes(64)
