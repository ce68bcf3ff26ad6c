"""GPU parity: the overlapped form of the fused first-layer dgrad + K4 (h2_occ_pp_kernel, the default behind dr_h2_dgrad_emb_sgd)
against the back-to-back form (DR_FUSED_K4_OVERLAP=0, h2_occ_nt_kernel<8>), bit for bit: tables, first-order weights, the gradient
rows of the non-unique slots in d_concat and the table's amax record, compared as SHA-256 digests of their bytes.  The switch is read once per process, so each form runs in a
child process of its own over the same seeded cases.  Unlike test_gpu_fused_k4.py (B <= 3000: one tile per block), the shapes here
give every block many tiles, so both wave groups take turns, and include tile counts that leave one group without a partner in
the last phase."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# B, F, V, K, ids ("uniform" / "zipf"), missing share, with lin_w, with table_amax
CASES = [
    (65536, 26, 60, 256, "uniform", 0.0, True, True),           # the bench shape, nearly every row shared
    (65536, 26, 150000, 256, "uniform", 0.0, True, True),       # the bench shape, mostly unique rows
    (65536 - 77, 26, 100000, 256, "uniform", 0.01, True, True), # M not a multiple of 128
    (65536 + 300, 26, 50000, 256, "uniform", 0.0, True, True),  # blocks with 15 and with 14 tiles: both last-phase cases
    (98304, 4, 100000, 256, "uniform", 0.0, True, True),        # one column tile, 3 tiles per block: an odd count everywhere
    (129, 3, 1000, 200, "uniform", 0.0, True, True),            # two row tiles, the second one row; K tail; ragged column tile
    (20000, 1, 5000, 256, "zipf", 0.05, True, True),            # F = 1
    (30000, 26, 100000, 200, "zipf", 0.03, False, False),       # Zipf + missing ids, K tail, no lin_w, no amax record
]


def _case(ops, B, F, V, K, kind, missing, with_lin, with_amax, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    if kind == "zipf":
        ids = np.minimum(rng.zipf(1.1, size=(B, F)) - 1, V - 1)
    else:
        ids = rng.integers(0, V, size=(B, F))
    if missing:
        ids[rng.random((B, F)) < missing] = -1
    ids = torch.as_tensor(ids).cuda()
    row_base = (torch.arange(F, dtype=torch.int64) * V).cuda()
    R, D = F * V, 64
    table = torch.randn((R, D), device="cuda", generator=g) * 0.125
    lin = torch.randn(R, device="cuda", generator=g) * 0.01 if with_lin else None
    in_dim = F * D + 13
    W = torch.randn((in_dim, K), device="cuda", generator=g) / in_dim ** 0.5
    dy = torch.randn((B, K), device="cuda", generator=g) * (torch.rand((B, K), device="cuda", generator=g) > 0.5) / B
    dl = torch.randn(B, device="cuda", generator=g) / B
    idc = ids.clamp_min(0) + row_base[None, :]
    sum_x = (table[idc] * (ids >= 0)[..., None]).sum(1).contiguous()
    lin_old_t = lin[idc].t().contiguous() if with_lin else None
    plan = ops.emb_sort_slots(ids, row_base, R)
    ids_t = ops.ids_transpose_i32(ids)
    wp = ops.H2WeightPlanes(W)
    dy_am = ops.h2_amax(dy)
    tab_am = ops.h2_amax(table) if with_amax else None
    d_concat = torch.zeros((B, (in_dim + 3) // 4 * 4), device="cuda")
    ops.h2_dgrad_emb_sgd(dy, dy_am, wp.w, ids_t, plan, row_base, table, lin, lin_old_t, sum_x, dl, -0.05, d_concat, table_amax=tab_am)
    torch.cuda.synchronize()
    uniq = int(plan.flags[:B * F].sum().item())
    return dict(table=_digest(table), lin=_digest(lin), d_concat=_digest(d_concat), amax=_digest(tab_am), uniq=uniq)


def _digest(t):
    """SHA-256 of a tensor's bytes (equal digests = bit-identical tensors; the results of a bench-shape case are gigabytes)"""
    if t is None:
        return None
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _child(out):
    sys.path.insert(0, ROOT)
    from deep_recommenders_amd import ops
    res = [_case(ops, *c, seed=101 + i) for i, c in enumerate(CASES)]
    with open(out, "w") as f:
        json.dump(res, f)


def _results(tmp_path, overlap):
    out = str(tmp_path / ("overlap%s.json" % overlap))
    env = dict(os.environ, DR_FUSED_K4_OVERLAP=overlap)
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, check=True, timeout=900)
    with open(out) as f:
        return json.load(f)


def test_overlapped_fused_dgrad_k4_is_bit_identical_to_the_back_to_back_kernel(tmp_path):
    new, old = _results(tmp_path, "1"), _results(tmp_path, "0")
    assert new[0]["uniq"] < 0.01 * 65536 * 26 and new[1]["uniq"] > 0.5 * 65536 * 26    # nearly all shared / mostly unique rows
    for c, a, b in zip(CASES, new, old):
        assert a["uniq"] == b["uniq"], c
        assert a["table"] == b["table"], c
        assert a["lin"] == b["lin"] and (a["lin"] is None) == (not c[6]), c
        assert a["d_concat"] == b["d_concat"], c                         # zero-initialised: the non-unique slots' rows, and nothing else
        assert a["amax"] == b["amax"] and (a["amax"] is None) == (not c[7]), c


@pytest.mark.parametrize("hidden", [[256, 64], [256, 128, 64]])
def test_engine_fused_k4_without_the_narrow_tail_matches_the_three_kernel_backward(hidden, monkeypatch):
    """Towers whose layer 1 has neither the narrow backward nor the one-pass tail, so no kernel above layer 0 leaves the dh0_amax
    record that layer 0's wgrad and dgrad read: the fused path must compute it itself, as the unfused path does (before, it read the
    record of the step before).  Fused (wgrad -> dgrad + K4's unique rows -> duplicate pass) against DR_FUSE_K4=0 (dgrad -> wgrad ->
    K4) over prefetched steps: the record, the tables, the first-order weights and bias, layer 0's W and b and the loss must be
    bit-identical after every step.  The layers above layer 0 take their bias gradients through float atomics (run-to-run
    differences in the last bits, fused or not), so after each comparison they are copied from one engine to the other: every step
    of the pair then starts from the same state."""
    from deep_recommenders_amd.engine import DeepFMEngine
    F, B, Nd, D, V = 6, 8192, 3, 64, 20000
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    batches = [(torch.randint(0, 10**12, (B, F), device="cuda", generator=g), torch.rand((B, Nd), device="cuda", generator=g),
                (torch.rand(B, device="cuda", generator=g) < 0.3).float()) for _ in range(3)]
    fused = DeepFMEngine(F, V, D, hidden, B, num_dense=Nd, lr=0.05, seed=3, lin_init_std=0.1)
    monkeypatch.setenv("DR_FUSE_K4", "0")
    plain = DeepFMEngine(F, V, D, hidden, B, num_dense=Nd, lr=0.05, seed=3, lin_init_std=0.1)
    assert fused.fuse_k4 and fused.h2 and not plain.fuse_k4
    assert not fused.fuse_tail and fused.narrow_ws[1] is None             # the case the record fix is for
    for n in range(4):
        k, d, l = batches[n % 3]
        nk, nd = batches[(n + 1) % 3][0], batches[(n + 1) % 3][1]
        l1 = float(fused.train_step(k, d, l, next_keys=nk, next_dense=nd).item())
        l0 = float(plain.train_step(k, d, l, next_keys=nk, next_dense=nd).item())
        torch.cuda.synchronize()
        assert l1 == l0, n
        assert torch.equal(fused.dh0_amax, plain.dh0_amax), n
        assert torch.equal(fused.table, plain.table), (n, int((fused.table != plain.table).sum().item()))
        assert torch.equal(fused.lin_w, plain.lin_w) and torch.equal(fused.lin_bias, plain.lin_bias), n
        assert torch.equal(fused.tab_amax, plain.tab_amax), n
        assert torch.equal(fused.Ws[0], plain.Ws[0]) and torch.equal(fused.bs[0], plain.bs[0]), n
        for i in range(1, len(plain.Ws)):
            plain.Ws[i].copy_(fused.Ws[i])
            plain.bs[i].copy_(fused.bs[i])


if __name__ == "__main__":
    _child(sys.argv[1])
