"""The engine-oracle helpers (tests/engine_oracle.py) have teeth -- no GPU needed.

A fp32 run of the oracle step (engine_oracle.HostEngine) stands in for the device at the `c2` and `fused` shapes of
tests/test_gpu_engine_matrix.py: unmodified it passes every check the matrix applies against the float64 step, and each planted error --
the ways an embedding kernel goes wrong without the loss noticing much -- fails one.  The Adam checks are measured on the same pair at
every Adam case's shape: what two correct implementations in two precisions differ by bounds what the constants may ask of a device.
"""
import numpy as np
import pytest
import torch

import engine_oracle as EO
from oracle import torch_ref as T

SHAPES = {                       # F, V, D, Nd, B, tower (the matrix's rows of the same names)
    "c2": (7, 10_000, 16, 0, 4096, [256, 32]),
    "fused": (4, 3000, 64, 3, 2304, [256, 32]),
}
STEPS = 3


def _data(shape, seed=20):
    """Three batches of per-field ids in [-1, V): 3 % missing, rows 0 and V - 1 of every field present, one whole example missing."""
    F, V, D, Nd, B, _ = SHAPES[shape]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(STEPS):
        ids = rng.integers(0, V, size=(B, F))
        ids[rng.random((B, F)) < 0.03] = -1
        ids[0], ids[1], ids[2] = 0, V - 1, -1
        dense = torch.from_numpy(rng.random((B, Nd), dtype=np.float32)) if Nd else None
        labels = torch.from_numpy((rng.random(B) < 0.3).astype(np.float32))
        out.append((ids, dense, labels))
    return out


def _edge_rows(F, V):
    m = np.zeros(F * V, dtype=bool)
    for f in range(F):
        m[[f * V, f * V + 1, f * V + V - 2, f * V + V - 1]] = True
    return m


def _run(shape, optimizer, lr, plant=None, host_ids=None, steps=STEPS):
    """The matrix's per-step sequence with the fp32 host engine as the device.  plant(host, before, orc64, i): edits the host's
    parameters after its step, as a wrong kernel would have left them.  host_ids: the ids the HOST trains on (default: the true ones)."""
    F, V, D, Nd, B, units = SHAPES[shape]
    data = _data(shape)
    ids_list = [d[0] for d in data]
    host = EO.HostEngine(F, V, D, Nd, B, units, optimizer, lr, seed=5)
    orc = EO._CompactOracle(host, ids_list, optimizer, lr, dtype=torch.float64, all_rows=True)
    ratios = {}
    for i, (ids, dense, labels) in enumerate(data[:steps]):
        orc.resync_from(host)
        before = (orc.table.float(), orc.lin.float(), orc.bias.float(), [w.float() for w in orc.Ws], [b.float() for b in orc.bs])
        loss, masks = host.train_step(host_ids if host_ids is not None else ids_list, i, dense, labels)
        if plant is not None:
            plant(host, before, orc, i)
        want = orc.step(i, dense, labels, relu_masks=masks)
        T.check_ties(orc.ties)
        assert abs(loss - want) <= 1e-5 * abs(want), (i, loss, want)
        touched = orc.touched(i)
        if optimizer == "sgd":
            EO._check_sgd_step(host, orc, before, touched, ratios, edge=_edge_rows(F, V))
        else:
            if optimizer == "adam":
                EO._assert_untouched("table rows", before[0].numpy(), host.table.numpy(), touched.numpy())
            EO._check_adam_step(host, orc, lr, i, ratios, touched=touched if optimizer == "adam" else None)
    return ratios


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fp32_step_passes_every_check(shape):
    ratios = _run(shape, "sgd", 1.0)
    print("%s: worst error / tolerance per parameter (fp32 against float64): %s" % (shape, {k: round(v, 4) for k, v in ratios.items()}))
    assert max(ratios.values()) < 1.0


def _rows_of(orc, i, pred):
    """compact rows of batch i's valid slots whose slot count satisfies pred"""
    c = orc.cidx[i][orc.valid[i]]
    rows, cnt = torch.unique(c, return_counts=True)
    return rows[pred(cnt)]


def _scaled_field(host, before, orc, i):
    lo, hi = 1 * orc.V, 2 * orc.V                                  # field 1's table gradient x 1.01
    host.table[lo:hi] = before[0][lo:hi] + 1.01 * (host.table[lo:hi] - before[0][lo:hi])


def _last_slot_wins(host, before, orc, i):
    g = host._orc.slot_grads[0]                                     # [B, F, D], the host's own per-slot gradients
    v = orc.valid[i].reshape(-1)
    c = orc.cidx[i].reshape(-1)[v]
    gt = torch.zeros_like(host.table)
    gt[c] = g.reshape(-1, orc.D)[v].float()                         # (no accumulation: one slot's gradient per row)
    host.table[c] = before[0][c] - host.lr * gt[c]


def _drop_last_row(host, before, orc, i):
    r = 2 * orc.V + orc.V - 1                                       # row V - 1 of field 2
    if not bool(orc.touched(i)[r]):
        raise RuntimeError("the batch does not look up row V - 1")
    host.table[r] = before[0][r]


def _double_lin_step(host, before, orc, i):
    r = _rows_of(orc, i, lambda cnt: cnt == 2)
    if len(r) <= 10:
        raise RuntimeError("too few rows with exactly two slots")
    host.lin_w[r] = before[1][r] + 2 * (host.lin_w[r] - before[1][r])


def _stray_ulp(host, before, orc, i):
    r = int(torch.nonzero(~orc.touched(i))[7])
    host.table[r, 3] = torch.nextafter(host.table[r, 3], torch.tensor(10.0))


PLANTS = {"field gradient x 1.01": _scaled_field, "duplicates not summed": _last_slot_wins, "row V-1 dropped": _drop_last_row,
          "first-order step twice on two-slot rows": _double_lin_step, "untouched row off by one ulp": _stray_ulp}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("plant", list(PLANTS))
def test_planted_error_fails(shape, plant):
    with pytest.raises(AssertionError) as e:
        _run(shape, "sgd", 1.0, plant=PLANTS[plant], steps=1)
    print("%s / %s fails with: %s" % (shape, plant, str(e.value)[:160]))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_missing_id_read_as_row_zero_fails(shape):
    bad = [np.maximum(d[0], 0) for d in _data(shape)]
    with pytest.raises(AssertionError) as e:
        _run(shape, "sgd", 1.0, host_ids=bad, steps=1)
    print("%s / missing id as row 0 fails with: %s" % (shape, str(e.value)[:160]))


@pytest.mark.parametrize("shape,optimizer", [("c2", "adam"), ("fused", "adam"), ("fused", "adam_tf")])
def test_adam_constants_hold_for_the_oracle_pair(shape, optimizer):
    """fp32 against float64, three Adam steps (lr 0.01) each from identical state, through _check_adam_step's constants unchanged.
    Measured (worst figure / its bound over the three steps, any parameter): c2 adam 2e-4, fused adam 3e-4, fused adam_tf 3e-4 -- the
    pair is far inside every constant at all three shapes, so the matrix applies them to the device as they are."""
    ratios = _run(shape, optimizer, 0.01)
    print("%s %s: worst figure / bound per parameter (fp32 against float64): %s" % (shape, optimizer, {k: round(v, 4) for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0
