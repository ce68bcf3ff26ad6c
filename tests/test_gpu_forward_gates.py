"""The two cross-stream events the next forward used to reach late, taken off its path -- both changes reorder launches and move no bit:

* dr_hash_sort_slots_parts: the prefetched chain (K1 + field-major ids + slot plan) issued in two parts, so that the forward's event can
  be recorded behind the launches that write the ids.  Part 1 then part 2 must leave every array the single call leaves, and part 1
  alone must already have left ids / ids_t.
* dr_emb_pool_bwd_dups_apply_refresh: W0's plane refresh as riders -- the blocks that step W0 inside K4's duplicate-pass launch store
  max |W0| per rider, rider blocks behind the hot rows' launch reduce those words, store the record and write both plane images.
  Against dr_emb_pool_bwd_dups_apply + hot rows + dr_h2_refresh_weight: W0, b0, record, planes bit for bit.
* DeepFMEngine over eight steps, new defaults against DR_IDS_EVENT=0 / DR_FOLD_REDUCES=1 and each switch alone.

Everything is compared as int32 / raw views: the same operations on the same values in the same order."""
import numpy as np
import pytest
import torch

D, V, N = 64, 1000, 256
LR = 0.05


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- the chain in two parts ---------------------------------------------------------------------------------------------------------------
def _poisoned_plan(ops, n):
    plan = ops.SortPlan(n, "cuda")
    plan.rows.fill_(-7)
    plan.slots.fill_(-7)
    plan.flags.fill_(0xAB)
    plan.dup_heads.fill_(-7)
    plan.dup_count.fill_(-7)
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("B,F,V_,trans", [(1000, 7, 5000, True), (77, 1, 50, False), (300, 65, 100, True), (130, 3, 1 << 40, True)])
def test_chain_in_two_parts_equals_the_single_call(ops, B, F, V_, trans):
    """Shapes: ragged example groups; one field without ids_t; F = 65 (no fused front kernel: part 1 is dr_hash_bucket_i64 +
    dr_ids_transpose_i32); 2^40 rows (no composite key: part 2 is the chip-wide radix sort).  Keys include negatives, -1 and a
    pass-through column.  All outputs start poisoned."""
    g = torch.Generator(device="cuda").manual_seed(B + F)
    keys = torch.randint(-(10**6), 10**15, (B, F), device="cuda", generator=g)
    keys[torch.rand((B, F), device="cuda", generator=g) < 0.05] = -1
    buckets = torch.full((F,), V_, dtype=torch.int64, device="cuda")
    if F > 2:
        buckets[2] = 0                                        # pass-through column: the key is the id
        keys[:, 2] = torch.randint(0, min(V_, 10**6), (B,), device="cuda", generator=g)
    row_base = torch.arange(F, dtype=torch.int64, device="cuda") * V_
    R = F * V_
    ids_ref = ops.hash_bucket_i64(keys, buckets)
    idt_ref = ops.ids_transpose_i32(ids_ref) if trans else None

    def outputs():
        return (torch.full_like(ids_ref, -7), torch.full((F, B), -7, dtype=torch.int32, device="cuda") if trans else None,
                _poisoned_plan(ops, B * F))
    ids0, idt0, plan0 = outputs()
    ops.hash_sort_slots(keys, buckets, row_base, R, ids0, idt0, plan0)
    ids1, idt1, plan1 = outputs()
    ops.hash_sort_slots(keys, buckets, row_base, R, ids1, idt1, plan1, parts=1)
    torch.cuda.synchronize()
    # part 1 alone: what the next forward reads is in place
    assert torch.equal(ids1, ids_ref)
    if trans:
        assert torch.equal(idt1, idt_ref)
    ops.hash_sort_slots(keys, buckets, row_base, R, ids1, idt1, plan1, parts=2)
    torch.cuda.synchronize()
    assert torch.equal(ids1, ids0) and torch.equal(ids0, ids_ref)
    if trans:
        assert torch.equal(idt1, idt0) and torch.equal(idt0, idt_ref)
    L = plan0.sorted_len()
    assert 0 <= L <= B * F and plan1.sorted_len() == L
    assert torch.equal(plan1.flags, plan0.flags)
    assert torch.equal(plan1.rows[:L], plan0.rows[:L]) and torch.equal(plan1.slots[:L], plan0.slots[:L])
    nh = int(plan0.dup_count[0].item())
    assert 0 <= nh <= B * F and int(plan1.dup_count[0].item()) == nh
    assert torch.equal(torch.sort(plan1.dup_heads[:nh]).values, torch.sort(plan0.dup_heads[:nh]).values)


# ---- the plane refresh as riders ------------------------------------------------------------------------------------------------------------
def _scene(R, F, nd, ragged_ld):
    K = F * D + nd
    g = torch.Generator(device="cuda").manual_seed(1000 * R + K)
    rng = np.random.default_rng(R + K)
    ids = rng.integers(0, V, size=(R, F))
    ids[rng.random((R, F)) < 0.05] = -1
    ids[: R // 2, 0] = 3                              # a row with more than 32 slots at R = 544: the hot rows' blocks have work too
    ids = torch.as_tensor(ids).cuda()
    s = dict(R=R, F=F, nd=nd, K=K, ids=ids, row_base=(torch.arange(F, dtype=torch.int64) * V).cuda(), ragged_ld=ragged_ld)
    s["table"] = torch.randn((F * V, D), device="cuda", generator=g) * 0.125
    s["lin"] = torch.randn(F * V, device="cuda", generator=g) * 0.01
    s["dense"] = None
    if nd:
        s["dense"] = torch.zeros((R, 32), device="cuda")
        s["dense"][:, :nd] = torch.rand((R, nd), device="cuda", generator=g)
    s["dy"] = torch.randn((R, N), device="cuda", generator=g) * (torch.rand((R, N), device="cuda", generator=g) > 0.5) / R
    W0 = torch.randn((K, N), device="cuda", generator=g) / K ** 0.5
    W0[K - 1, N - 3] = 7.0                            # the maximum, in the range of the last rider (a partial one unless 4 | K)
    W0[K // 2, 5] = 1e15                              # ... after the first call shrinks this one
    s["W0"] = W0
    s["b0"] = torch.randn(N, device="cuda", generator=g) * 0.1
    s["dl"] = torch.randn(R, device="cuda", generator=g) / R
    s["d_concat"] = torch.randn((R, (K + 3) // 4 * 4), device="cuda", generator=g) / R
    idc = ids.clamp_min(0) + s["row_base"][None, :]
    s["sum_x"] = (s["table"][idc] * (ids >= 0)[..., None]).sum(1).contiguous()
    s["lin_old_t"] = s["lin"][idc].t().contiguous()
    return s


def _two_steps(ops, s, riders, det=True):
    """Two consecutive first-layer steps (wgrad's main launch, duplicate pass with the reduce riding, hot rows, plane refresh); between
    them W0's largest element is taken down from outside.  Returns after each step: W0, b0, table, record, both images, the spare image.
    det=False: no scratch rows (and so no FM term) -- the hot rows have no parked pieces to combine, as with DR_K4_DETERMINISTIC=0, and
    the second launch consists of the refresh's riders alone."""
    R, F, K = s["R"], s["F"], s["K"]
    if s["ragged_ld"]:                                # row stride 257, a base 4 bytes past a 16-byte boundary: the one-column reduce
        W0 = torch.zeros(K * (N + 1) + 1, device="cuda")[1:].view(K, N + 1)[:, :N]
        W0.copy_(s["W0"])
    else:
        W0 = s["W0"].clone()
    b0 = s["b0"].clone()
    table, lin, bias = s["table"].clone(), s["lin"].clone(), torch.zeros(1, device="cuda")
    plan = ops.emb_sort_slots(s["ids"], s["row_base"], F * V)
    ids_t = ops.ids_transpose_i32(s["ids"])
    den_am = ops.h2_amax(s["dense"]) if s["dense"] is not None else None
    dy_am = ops.h2_amax(s["dy"])
    tab_am = ops.h2_amax(table)
    ws = ops.bf3_wgrad_workspace(R, K, N, "cuda").fill_(float("nan"))
    xs = torch.full((R * F, D), float("nan"), device="cuda") if det else None
    sum_x = s["sum_x"] if det else None
    wp = ops.H2WeightPlanes(W0, double_buffer=True)
    out = []
    for step in range(2):
        ops.h2_wgrad_emb(ids_t, s["row_base"], table, tab_am, s["dense"], den_am, s["dy"], dy_am, -LR, W0, b0, workspace=ws, parts=1)
        tgt = None
        if riders:
            tgt = wp.hand_off()
            tgt[3].fill_(-1)                          # stale words and a stale record: 0xFFFFFFFF would win every maximum
            tgt[2].fill_(-1)
        for parts in (1, 2):
            if parts == 1 or riders:
                ops.emb_pool_bwd_dups_apply(s["ids"], s["row_base"], plan, D, F * V, s["d_concat"], s["dl"], -LR, table, lin, bias, sum_x,
                                            xs, s["lin_old_t"], tab_am, ws, R, -LR, W0, b0, wg_h2=True, parts=parts, refresh=tgt)
            else:
                ops.emb_pool_bwd_sorted(s["ids"], s["row_base"], plan, D, F * V, s["d_concat"], s["dl"], -LR, table, lin, bias,
                                        sum_x=sum_x, x_sorted=xs, parts=2 | 8, lin_old_t=s["lin_old_t"], table_amax=tab_am)
        if not riders:
            wp.amax.fill_(-1)
            wp._w_alt.amax.fill_(-1)
            wp.refresh()
        torch.cuda.synchronize()
        out.append(dict(W0=W0.clone(), b0=b0.clone(), table=table.clone(), rec=wp.amax.clone(), w=wp.w.buf.clone(), wt=wp.wt.buf.clone(),
                        spare=wp._w_alt.buf.clone()))
        W0[K // 2, 5] = 0.5                           # the maximum shrinks: the next record must come down
    return out


RIDER_SHAPES = [(R, F, nd, False) for R in (32, 544) for (F, nd) in ((1, 0), (3, 5), (26, 13))] + [(32, 26, 13, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("R,F,nd,ragged_ld", RIDER_SHAPES)
def test_refresh_riders_give_the_two_launch_refreshs_bits(ops, R, F, nd, ragged_ld):
    """K = 64 (16 riders, all full), 197 and 1677 (last rider partial), B = 32 and 544.  The last case reaches the riders' loop: an
    unaligned W0 takes the one-column reduce, 1677 logical blocks on 1024 riders."""
    s = _scene(R, F, nd, ragged_ld)
    ref, new = _two_steps(ops, s, False), _two_steps(ops, s, True)
    K = s["K"]
    for n, (a, b) in enumerate(zip(ref, new)):
        assert bool(torch.isfinite(b["W0"]).all())
        for k in ("W0", "b0", "table", "rec", "w", "wt", "spare"):
            assert torch.equal(_bits(b[k]), _bits(a[k])), "call %d: %s" % (n, k)
    assert not torch.equal(ref[0]["W0"], s["W0"])                                          # the step did move the layer
    rec = [int(r["rec"].item()) for r in new]
    assert rec[0] == int(new[0]["W0"].abs().max().view(torch.int32).item()) and new[0]["W0"].abs().max().item() > 9e14
    # second call: the record came down to the element in the last rider's range
    assert rec[1] < rec[0] and rec[1] == int(new[1]["W0"][K - 1, N - 3].abs().view(torch.int32).item())
    assert 6.0 < new[1]["W0"].abs().max().item() < 8.0
    assert not torch.equal(new[1]["w"], new[0]["w"])


@pytest.mark.gpu
def test_refresh_riders_alone_in_the_second_launch(ops):
    """Without scratch rows the hot rows' blocks are not launched (what DR_K4_DETERMINISTIC=0 does to the engine's step): the second launch
    is the riders alone and still leaves the record and both images.  R = 32: no row has more than 32 slots, every path is reproducible."""
    s = _scene(32, 3, 5, False)
    ref, new = _two_steps(ops, s, False, det=False), _two_steps(ops, s, True, det=False)
    for n, (a, b) in enumerate(zip(ref, new)):
        for k in ("W0", "b0", "table", "rec", "w", "wt", "spare"):
            assert torch.equal(_bits(b[k]), _bits(a[k])), "call %d: %s" % (n, k)
    assert int(new[1]["rec"].item()) < int(new[0]["rec"].item()) and not torch.equal(new[1]["w"], new[0]["w"])


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------
def _engine_run(monkeypatch, env, narrow_ids):
    from deep_recommenders_amd.engine import DeepFMEngine
    for k in ("DR_IDS_EVENT", "DR_FOLD_REDUCES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, F, Nd = 2048, 3, 5
    g = torch.Generator(device="cuda").manual_seed(11)
    hi = 50 if narrow_ids else 10**12
    bt = [(torch.randint(0, hi, (B, F), device="cuda", generator=g), torch.rand((B, Nd), device="cuda", generator=g),
           (torch.rand(B, device="cuda", generator=g) < 0.3).float()) for _ in range(8)]
    eng = DeepFMEngine(F, 100000, D, [256, 32], B, num_dense=Nd, lr=LR, seed=3, lin_init_std=0.1)
    snaps = []

    def snap():
        torch.cuda.synchronize()
        wp = eng.wplanes[0]
        snaps.append([t.clone() for t in (eng.loss, eng.table, eng.lin_w, eng.flat_params, wp.w.buf, wp.wt.buf, wp.amax, eng.prob)])

    def step(n, nxt):
        k, d, l = bt[n]
        eng.train_step(k, d, l, next_keys=None if nxt is None else bt[nxt][0], next_dense=None if nxt is None else bt[nxt][1])
        snap()
    step(0, 1)
    step(1, 2)
    step(2, 0)                                        # a wrong next_keys: the next step discards the prefetch ...
    step(3, None)                                     # ... and prefetches nothing itself
    step(4, 5)
    eng.Ws[0].mul_(0.5)                               # an outside write: the forward re-splits W0 (ensure_fresh), two launches
    step(5, 6)
    step(6, 7)
    step(7, None)
    eng.forward(*bt[0])                               # outside train_step: reads the planes the last step's riders wrote
    snap()
    return eng, snaps


ENGINE_WHAT = ("loss", "table", "lin_w", "flat_params", "w planes", "wt planes", "record", "prob")


@pytest.fixture(scope="module", params=[False, True], ids=["wide_ids", "50_ids_large_path"])
def engine_runs(request, ops):
    """The four switch settings over the same eight steps.  50 ids per field with the LDS sort disabled: every batch takes the plan's
    LARGE path, the longest chain tail."""
    mp = pytest.MonkeyPatch()
    prev = ops.emb_plan_set_small_limit(0) if request.param else None
    try:
        runs = {name: _engine_run(mp, env, request.param) for name, env in (
            ("new", {}), ("old", {"DR_IDS_EVENT": "0", "DR_FOLD_REDUCES": "1"}),
            ("ids_only", {"DR_FOLD_REDUCES": "1"}), ("planes_only", {"DR_IDS_EVENT": "0"}))}
    finally:
        mp.undo()
        if prev is not None:
            ops.emb_plan_set_small_limit(prev)
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["new", "ids_only", "planes_only"])
def test_engine_steps_are_bit_identical_with_the_gates_moved(engine_runs, arm):
    old, s_old = engine_runs["old"]
    eng, s_new = engine_runs[arm]
    assert old.fold_reduces and not old.fold_planes and not old.ids_event_early and old.fuse_k4 and old.tail_in_fwd
    assert eng.fold_reduces and eng.fold_planes == (arm != "ids_only") and eng.ids_event_early == (arm != "planes_only")
    assert len(s_new) == len(s_old) == 9
    for n, (a, b) in enumerate(zip(s_new, s_old)):
        for x, y, what in zip(a, b, ENGINE_WHAT):
            assert torch.equal(_bits(x), _bits(y)), "step %d: %s" % (n, what)
    assert all(bool(torch.isfinite(s[0]).all()) for s in s_new)
    assert not torch.equal(s_new[0][3], s_new[1][3]) and not torch.equal(s_new[0][4], s_new[1][4])    # weights and planes do move
