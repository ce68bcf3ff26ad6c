"""Every DeepFMEngine kernel path against a float64 oracle step.

DeepFMEngine.__init__ picks the step's kernels from about fifteen gates that depend on F, V, D, the dense-feature count, the tower
widths, B, the optimizer and two process-wide GEMM switches.  The bench shape has its oracle test (tests/test_gpu_benchcfg.py, tables of
6 - 66 GB) and so has a toy with every gate off (tests/test_gpu_models.py); the other arrangements were only ever compared bit for bit
with one another.  Here each row of CASES builds a small engine, ASSERTS the gates of its row (a case must not pass on another path),
and runs three training steps -- the first not prefetched, the other two prefetched on either of the double buffers -- each against one
float64 oracle step from the device's own state (tests/engine_oracle.py; oracle/torch_ref.py under autograd, with the device's ReLU
decisions and T.check_ties):

  ids      bit-exact (oracle/tf_semantics.py hash_bucket_i64, or the input itself with hashed=False)
  loss     1e-5 relative (the project's north-star figure)
  SGD      every parameter through _assert_update with its constants; rows the batch did not look up bit-identical -- for the small
           tables that is EVERY other row of the table; the first and last two rows of every field once more on their own
  Adam     _check_adam_step with its constants on the rows the step looked up (tests/test_engine_oracle_cpu.py measures the fp32 /
           float64 oracle pair against the same constants at these shapes: at most 3e-4 of any bound)
  and the oracle's own update of every parameter is at least 100 fp32 spacings of the parameter's rms magnitude (not vacuous).

After the third step the evaluation forward (eng.forward outside train_step, other kernels than the training forward wherever the
tail is fused) is compared with the sigmoid of the float64 logit from the device's current parameters: the project's logit tolerance
is 1e-5 (test_estimator_fm_and_deepfm) and |d sigmoid| <= |d logit| / 4, so |d prob| <= 2.5e-6.

SGD runs at lr 1.0 (see tests/test_gpu_benchcfg.py: at 0.01 a row's update is below the fp32 spacing of the row), Adam at 0.01.
The three v24 cases place ids within two rows of the 24-bit row limits of the fused first layer (V <= 2^24) and of the gathering
wgrad / fused K4 (V < 2^24 - 1): 8.6 GB of table each; the host sees the rows the batches touch and a sample of >= 10 000 others.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine_oracle as EO
from oracle import tf_semantics as O
from oracle import torch_ref as T

FUSED = ["h2", "fuse_k3", "no_concat", "tail_in_fwd", "fuse_k4", "fold_reduces", "fold_planes"]
_S = dict(F=4, V=3000, D=64, Nd=3, tower=[256, 32], B=2304)                       # the "same" of the rows below


def _case(on, off=(), **kw):
    c = dict(_S, opt="sgd", hashed=True, ids=None, split=None, mode=None, on=list(on), off=list(off))
    c.update(kw)
    return c


_C2 = dict(F=7, V=10_000, D=16, Nd=0, tower=[256, 32], B=4096, ids="bench",
           on=["wplanes0", "fuse_head", "narrow1", "fuse_tail"], off=["fuse_k3", "h2", "no_concat", "fuse_k4"])
CASES = {
    "c2": _case(**_C2),                                                              # bench.py --preset c2
    "c2-adam": _case(**dict(_C2, opt="adam")),
    "fused": _case(FUSED),
    "fused-r32": _case(FUSED, B=2080),                                               # 65 x 32 rows: a ragged 256-row tile
    "fused-odd": _case(["h2", "fuse_k4", "fuse_head"], ["narrow_any", "fuse_tail", "tail_in_fwd", "fold_reduces"], B=2050),
    "nodense": _case(FUSED, ["dense_pads"], Nd=0),
    "dense40": _case(["wplanes0", "fuse_tail"], ["fuse_k3", "h2", "no_concat"], F=3, V=5000, Nd=40, tower=[256, 16]),
    "wide1": _case(["h2", "fuse_k4"], ["fuse_head", "narrow1"], tower=[256, 64]),
    "deep-a": _case(["h2", "fuse_k4", "fuse_head", "fuse_tail", "wplanes1"], ["tail_in_fwd", "narrow1"], tower=[256, 128, 32]),
    "deep-b": _case(["h2", "fuse_k4", "wplanes1"], ["fuse_head"], tower=[256, 128, 64]),
    "adam": _case(["h2", "no_concat", "fuse_tail"], ["fuse_k4", "tail_in_fwd"], opt="adam"),
    "adam-tf": _case(["fuse_k3", "no_concat"], ["h2"], opt="adam_tf"),
    "bf16x3": _case(["fuse_k3", "no_concat"], ["h2", "fuse_k4", "tail_in_fwd"], split="bf16x3"),
    "native": _case(["fuse_k3"], ["wplanes_any", "no_concat", "h2"], mode="native"),
    "d32": _case(["wplanes0"], ["fuse_k3"], D=32),
    "d8": _case(["wplanes0"], ["fuse_k3"], F=8, D=8),                                # in_dim 67
    "small": _case(["fuse_head", "fuse_tail"], ["wplanes_any"], B=480),
    "ids": _case(FUSED, hashed=False, ids="missing"),
    "hot": _case(FUSED, hashed=False, ids="hot"),
    "v24-2": _case(FUSED, F=2, V=(1 << 24) - 2, hashed=False, ids="edge"),
    "v24": _case(["fuse_k3"], ["no_concat", "h2"], F=2, V=1 << 24, hashed=False, ids="edge"),
    "v24+1": _case([], ["fuse_k3"], F=2, V=(1 << 24) + 1, hashed=False, ids="edge"),
}


def _gates(eng):
    g = {k: bool(getattr(eng, k)) for k in ("fuse_k3", "no_concat", "h2", "tail_in_fwd", "fuse_k4", "fold_reduces", "fold_planes",
                                            "fuse_head", "fuse_tail")}
    g["wplanes0"] = eng.wplanes[0] is not None
    g["wplanes1"] = len(eng.wplanes) > 1 and eng.wplanes[1] is not None
    g["wplanes_any"] = any(w is not None for w in eng.wplanes)
    g["narrow1"] = eng.narrow_ws[1] is not None
    g["narrow_any"] = any(w is not None for w in eng.narrow_ws)
    g["dense_pads"] = eng._dense_pads is not None
    return g


def _batches(c, seed=1234):
    """Three batches (keys, dense, labels) on the device and the per-field ids [B, F] the engine must derive from the keys."""
    F, V, Nd, B = c["F"], c["V"], c["Nd"], c["B"]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    out, ids_list = [], []
    for _ in range(3):
        if c["ids"] == "bench":                                                      # bench.py:synth_batches
            keys = torch.randint(0, 10**16, (B, F), device="cuda", generator=g)
        elif c["ids"] is None:
            keys = torch.randint(0, 10**12, (B, F), device="cuda", generator=g)
        else:
            if c["ids"] == "hot":                                                    # a few rows shared by hundreds of slots
                ids = np.minimum((rng.pareto(1.05, size=(B, F)) * 3).astype(np.int64), V - 1)
            else:
                ids = rng.integers(0, V, size=(B, F))
            if c["ids"] == "missing":
                ids[rng.random((B, F)) < 0.03] = -1
                ids[0], ids[1], ids[2] = 0, V - 1, -1                                # both end rows of every field; one example all missing
            if c["ids"] == "edge":
                ids[0], ids[1], ids[2], ids[3] = 0, 1, V - 2, V - 1
            keys = torch.as_tensor(ids).cuda()
        if c["hashed"]:
            k = keys.cpu().numpy()
            ids_list.append(np.stack([O.hash_bucket_i64(k[:, f], V) for f in range(F)], axis=1))
        else:
            ids_list.append(keys.cpu().numpy())
        dense = torch.rand((B, Nd), device="cuda", generator=g) if Nd else None
        labels = (torch.rand(B, device="cuda", generator=g) < (0.25 if c["ids"] == "bench" else 0.3)).float()
        out.append((keys, dense, labels))
    return out, ids_list


def _run_case(name, c):
    from deep_recommenders_amd.engine import DeepFMEngine
    F, V, D, Nd, B, opt = c["F"], c["V"], c["D"], c["Nd"], c["B"], c["opt"]
    lr = 1.0 if opt == "sgd" else 0.01
    big = F * V > (1 << 22)
    eng = DeepFMEngine(F, V, D, c["tower"], B, num_dense=Nd, lr=lr, seed=42, hashed=c["hashed"], lin_init_std=0.1, optimizer=opt)
    gates = _gates(eng)
    wrong = [k for k in c["on"] if not gates[k]] + ["not " + k for k in c["off"] if gates[k]]
    assert not wrong, "%s runs on another path than its row says: %s" % (name, wrong)
    batches, ids_list = _batches(c)
    if c["ids"] == "hot":
        cnt = np.unique(ids_list[0] + np.arange(F, dtype=np.int64)[None, :] * V, return_counts=True)[1]
        assert (cnt > 32).any() and (cnt == 2).any(), "the batch has no row for K4's parked-pieces path / no row with exactly two slots"
    orc = EO._CompactOracle(eng, ids_list, opt, lr, dtype=torch.float64, all_rows=not big)
    ends = np.concatenate([f * V + np.array([0, 1, V - 2, V - 1], dtype=np.int64) for f in range(F)])
    edge = np.isin(orc.U, ends)
    if big:
        # rows outside the touched set: a random sample and the neighbours of the forced end rows, all to stay bit-identical
        near = np.concatenate([ends + d for d in (-2, -1, 1, 2)])
        cand = np.concatenate([near[(near >= 0) & (near < F * V)], torch.randint(0, F * V, (40000,), generator=torch.Generator().manual_seed(5)).numpy()])
        cand = np.unique(cand[~np.isin(cand, orc.U)])
        assert cand.size >= 10000
        untouched = torch.from_numpy(cand).cuda()
        un_t0, un_l0 = eng.table[untouched].clone(), eng.lin_w[untouched].clone()
    ratios = {}
    f32 = lambda t: t.float().numpy()
    for i, (keys, dense, labels) in enumerate(batches):
        orc.resync_from(eng)                                  # every step is a one-step comparison from the device's own state
        before = (orc.table.float(), orc.lin.float(), orc.bias.float(), [w.float() for w in orc.Ws], [b.float() for b in orc.bs])
        nk, nd = (batches[i + 1][0], batches[i + 1][1]) if i + 1 < len(batches) else (None, None)
        loss = float(eng.train_step(keys, dense, labels, next_keys=nk, next_dense=nd).item())
        assert eng._plan_prefetched == (i > 0), "the prefetched plan was not picked up"
        np.testing.assert_array_equal(eng.ids.cpu().numpy(), ids_list[i])                     # integer path: bit-exact
        masks = EO._device_relu_masks(eng)
        if opt == "adam_tf":
            eng.adam_flush()                                  # every row up to date: the oracle is TF's dense Adam on ALL rows
        want = orc.step(i, dense.cpu() if dense is not None else None, labels.cpu(), relu_masks=masks)
        T.check_ties(orc.ties, max_frac=1e-5 if opt == "sgd" else 1e-4)
        assert abs(loss - want) <= 1e-5 * abs(want), (i, loss, want)                          # north_star: 1e-5 relative
        touched = orc.touched(i)
        if opt == "sgd":
            EO._check_sgd_step(eng, orc, before, touched, ratios, edge=edge)
        else:
            tm = touched.numpy() if opt == "adam" else np.ones(len(orc.U), dtype=bool)
            tmt = torch.from_numpy(tm)
            if opt == "adam":                                 # row-wise Adam: a row at rest does not move
                EO._assert_untouched("table rows", f32(before[0]), eng.table[orc.Ud].cpu().numpy(), tm)
                EO._assert_untouched("first-order weights", f32(before[1]), eng.lin_w[orc.Ud].cpu().numpy(), tm)
            for nm, b_, w_ in [("table", before[0][tmt], orc.table[tmt]), ("lin", before[1][tmt], orc.lin[tmt]), ("bias", before[2], orc.bias)] + \
                    [("W%d" % j, before[3][j], orc.Ws[j]) for j in range(len(orc.Ws))] + [("b%d" % j, before[4][j], orc.bs[j]) for j in range(len(orc.bs))]:
                EO._assert_not_vacuous(nm, f32(b_), w_.numpy())
            EO._check_adam_step(eng, orc, lr, i, ratios, touched=touched if opt == "adam" else None)
    torch.cuda.synchronize()
    if big:
        assert torch.equal(eng.table[untouched], un_t0) and torch.equal(eng.lin_w[untouched], un_l0), "an untouched row changed"
    print("%s: worst error / tolerance per parameter over 3 steps: %s" % (name, {k: round(v, 3) for k, v in ratios.items()}))
    if opt != "adam_tf":                                      # (adam_tf's forward stamps rows: it is valid inside train_step only)
        keys, dense, labels = batches[-1]
        prob = eng.forward(keys, dense, None).double().cpu()
        orc.resync_from(eng)
        with torch.no_grad():
            want_p = torch.sigmoid(orc.logit(len(batches) - 1, dense.cpu() if dense is not None else None))
        err = float((prob - want_p).abs().max())
        print("%s: evaluation forward, worst |prob - sigmoid(float64 logit)| %.3e (bound 2.5e-6)" % (name, err))
        assert err <= 1e-5 / 4, (name, err)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(CASES))
def test_engine_step_matches_float64_oracle(name):
    from deep_recommenders_amd import ops
    c = CASES[name]
    if c["F"] * c["V"] > (1 << 22):
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < 24e9:
            pytest.skip("needs 24 GB of free device memory for an 8.6 GB table, its initialisation and the step's buffers")
    prev_split = ops.set_gemm_split(c["split"]) if c["split"] else None
    prev_mode = ops.set_gemm_mode(c["mode"]) if c["mode"] else None
    try:
        _run_case(name, c)
    finally:
        if prev_split is not None:
            ops.set_gemm_split(prev_split)
        if prev_mode is not None:
            ops.set_gemm_mode(prev_mode)
