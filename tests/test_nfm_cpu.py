"""NFM without a GPU: the float64 restatement (tests/nfm_ref.py) against autograd and against itself, the derived error bounds against
its own float32 run, every host-side domain error of the ops.bi_interaction_* wrappers and of the model's constructor, the C header, and
the absence of a new autograd Function."""
import inspect
import os
import re

import pytest
import torch

import nfm_ref as R
from deep_recommenders_amd import feature_column as fc
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking import NFM, BiInteraction     # the feature: without it this file does not import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dr_bi_interact_fwd", "dr_bi_interact_bwd", "dr_bi_interact_gather_fwd", "dr_bi_interact_gather_bwd"]


@pytest.mark.parametrize("shape", R.SHAPES[:-1], ids=str)
def test_closed_form_backward_equals_float64_autograd(shape):
    c = R.make_case(*shape)
    rows = R.gather(c["table"], c["ids"], c["row_base"]).requires_grad_()
    out = R.bi_forward(rows)
    assert (out - R.bi_pairs(rows)).abs().max().item() <= 1e-12 * max(1.0, out.abs().max().item())   # the two ways to write it
    out.backward(c["d_out"])
    want = rows.grad
    got = R.bi_backward(rows.detach(), c["d_out"])
    assert (got - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())


def test_one_field_is_exactly_zero_and_a_missing_id_is_a_row_of_zeros():
    c = R.make_case(3, 1, 4)
    rows = R.gather(c["table"], c["ids"], c["row_base"])
    assert (R.bi_forward(rows) == 0).all()
    assert (rows[1, 0] == 0).all() and c["ids"][1, 0] == -1
    c = R.make_case(4, 3, 8)
    assert (R.gather(c["table"], c["ids"], c["row_base"])[2, 1] == 0).all()


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_the_derived_bounds_hold_for_the_float32_run_of_the_restatement(shape):
    """the bounds hold for any summation order, so they hold for torch's; read here at most 0.28 forward, 0.40 backward"""
    c = R.make_case(*shape)
    rows = R.gather(c["table"], c["ids"], c["row_base"])
    out32 = R.bi_forward(rows.float()).double()
    bound = R.fwd_bound(rows)
    err = (out32 - R.bi_forward(rows)).abs()
    assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max().item()
    d32 = R.bi_backward(rows.float(), c["d_out"].float()).double()
    bound = R.bwd_bound(rows, c["d_out"])
    err = (d32 - R.bi_backward(rows, c["d_out"])).abs()
    assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max().item()
    bags = [c["ids"][:, f:f + 1] for f in range(shape[1])]
    fo32 = R.first_order(c["lin_w"].float(), c["lin_bias"].float(), bags, c["row_base"]).double()
    err = (fo32 - R.first_order(c["lin_w"], c["lin_bias"], bags, c["row_base"])).abs()
    assert (err <= R.first_order_bound(c["lin_w"], c["lin_bias"], bags, c["row_base"])).all()


@pytest.mark.parametrize("shape", [(4, 3, 8), (5, 26, 64)], ids=str)
def test_integer_grids_are_exact_in_float32(shape):
    c = R.make_case(*shape, grid=True)
    rows = R.gather(c["table"], c["ids"], c["row_base"])
    assert torch.equal(R.bi_forward(rows.float()).double(), R.bi_forward(rows))
    assert torch.equal(R.bi_backward(rows.float(), c["d_out"].float()).double(), R.bi_backward(rows, c["d_out"]))


def test_the_float64_step_lowers_the_loss():
    torch.manual_seed(0)
    F, D = 3, 4
    params = {"table": 0.3 * torch.randn(15, D, dtype=torch.float64), "lin_w": torch.zeros(15, dtype=torch.float64),
              "lin_bias": torch.zeros(1, dtype=torch.float64), "kernels": [0.5 * torch.randn(D, 8, dtype=torch.float64)],
              "biases": [torch.zeros(8, dtype=torch.float64)], "w_out": 0.5 * torch.randn(8, 1, dtype=torch.float64)}
    ids = torch.randint(0, 5, (32, F))
    bags = [ids[:, f:f + 1] for f in range(F)]
    y = torch.randint(0, 2, (32,)).double()
    base = 5 * torch.arange(F)
    losses = []
    for _ in range(20):
        params, loss = R.train_step(params, bags, base, y, 0.5)
        losses.append(loss.item())
    assert losses[-1] < losses[0]


def _rows(B=2, F=3, D=8):
    return torch.zeros(B, F * D)


@pytest.mark.parametrize("F, D", [(0, 8), (1025, 8), (3, 0), (3, 6), (3, 260), (3, 2)])
def test_dims_outside_the_domain_are_value_errors(F, D):
    with pytest.raises(ValueError, match="bi_interaction"):
        ops.bi_interaction_fwd(torch.zeros(2, max(F * D, 1)), F, D)
    with pytest.raises(ValueError, match="bi_interaction"):
        ops.bi_interaction_gather_fwd(torch.zeros(2, max(F, 1), dtype=torch.int64), torch.zeros(max(F, 1), dtype=torch.int64),
                                      torch.zeros(4, max(D, 1)), F, D)


def test_every_argument_error_is_raised_on_the_host():
    F, D = 3, 8
    ids, base, table = torch.zeros(2, F, dtype=torch.int64), torch.zeros(F, dtype=torch.int64), torch.zeros(5, D)
    bad = [
        lambda: ops.bi_interaction_fwd(_rows().double(), F, D),                                    # dtype
        lambda: ops.bi_interaction_fwd(torch.zeros(2, F * D + 4), F, D),                            # width
        lambda: ops.bi_interaction_fwd(torch.zeros(2, F, D + 4), F, D),                             # 3-d shape
        lambda: ops.bi_interaction_fwd(torch.zeros(2, 2 * F * D)[:, ::2], F, D),                    # column stride
        lambda: ops.bi_interaction_fwd(torch.zeros(3, F * D + 2)[:, :F * D], F, D),                 # pitch not a multiple of 4
        lambda: ops.bi_interaction_fwd(_rows(), F, D, out=torch.zeros(3, D)),                       # out rows
        lambda: ops.bi_interaction_fwd(_rows(), F, D, out=torch.zeros(2, D + 4)),                   # out width
        lambda: ops.bi_interaction_bwd(_rows(), F, D, torch.zeros(2, D + 4)),                       # d_out width
        lambda: ops.bi_interaction_bwd(_rows(), F, D, torch.zeros(3, D)),                           # d_out rows
        lambda: ops.bi_interaction_bwd(_rows(), F, D, torch.zeros(2, D), d_rows=torch.zeros(3, F * D)),
        lambda: ops.bi_interaction_bwd(_rows(), F, D, torch.zeros(2, D), d_rows=torch.zeros(2, F * D).double()),
        lambda: ops.bi_interaction_gather_fwd(ids.int(), base, table, F, D),                        # ids dtype
        lambda: ops.bi_interaction_gather_fwd(ids[:, :2], base, table, F, D),                       # ids width
        lambda: ops.bi_interaction_gather_fwd(ids, base[:2], table, F, D),                          # row_base length
        lambda: ops.bi_interaction_gather_fwd(ids, base, torch.zeros(5, D + 4), F, D),              # table width
        lambda: ops.bi_interaction_gather_fwd(ids, base, torch.zeros(5, 2 * D)[:, :D], F, D),       # table pitch
        lambda: ops.bi_interaction_gather_fwd(ids, base, table, F, D, lin_w=torch.zeros(4)),        # lin_w length
        lambda: ops.bi_interaction_gather_fwd(ids, base, table, F, D, lin_w=torch.zeros(5), lin_bias=torch.zeros(2)),
        lambda: ops.bi_interaction_gather_bwd(ids, base, table, F, D, torch.zeros(2, D + 4)),
        lambda: ops.bi_interaction_gather_bwd(ids, base, table, F, D, torch.zeros(2, D), d_rows=torch.zeros(2, F * D + 4)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert i >= 0


def test_valid_arguments_reach_the_device_boundary_and_stop_there():
    """on a machine without a GPU a well-formed call fails at the first device pointer, with the package's own message"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bi_interaction_fwd(_rows(), 3, 8)


def _columns(n=3, dim=8, buckets=5):
    cats = [fc.categorical_column_with_identity("f%d" % i, buckets) for i in range(n)]
    return [fc.indicator_column(c) for c in cats], [fc.embedding_column(c, dim) for c in cats]


def test_constructor_errors():
    ind, emb = _columns()
    with pytest.raises(ValueError, match="indicator"):
        NFM([], emb, [8], device="cpu")
    with pytest.raises(ValueError, match="dnn_units_size"):
        NFM(ind, emb, [], device="cpu")
    with pytest.raises(ValueError, match="dnn_units_size"):
        NFM(ind, emb, [8, 0], device="cpu")
    with pytest.raises(ValueError, match="activation"):
        NFM(ind, emb, [8], activation="gelu", device="cpu")
    with pytest.raises(ValueError, match="dropout"):
        NFM(ind, emb, [8], dropout=1.0, device="cpu")
    with pytest.raises(ValueError, match="bi_dropout"):
        NFM(ind, emb, [8], bi_dropout=-0.1, device="cpu")
    with pytest.raises(ValueError):
        NFM(ind, _columns(dim=6)[1], [8], device="cpu")                    # D % 4
    model = NFM(ind, emb, [16, 8], dropout=0.1, device="cpu")
    assert [tuple(k.shape) for k in model.kernels] == [(8, 16), (16, 8)] and tuple(model.w_out.shape) == (8, 1)
    assert model.get_config()["dnn_units_size"] == [16, 8]
    assert "DO NOT REACH THE SLAB" in NFM.__doc__
    with pytest.raises(ValueError, match="missing"):
        model.logits({"f0": [[1]], "f1": [[1]]})
    with pytest.raises(ValueError, match="dim"):
        BiInteraction().call(torch.zeros(4))
    with pytest.raises(ValueError, match="num_fields"):
        BiInteraction().call(torch.zeros(2, 24))
    with pytest.raises(ValueError, match="bi_interaction"):
        BiInteraction().call(torch.zeros(2, 3, 6))


def test_the_header_declares_the_entry_points():
    from deep_recommenders_amd import _cabi
    protos = _cabi.prototypes(os.path.join(ROOT, "include", "dr_hotpath.h"))
    for s in SYMBOLS:
        assert s in protos, s
    assert len(protos["dr_bi_interact_fwd"][1]) == 8 and len(protos["dr_bi_interact_bwd"][1]) == 10
    assert len(protos["dr_bi_interact_gather_fwd"][1]) == 12 and len(protos["dr_bi_interact_gather_bwd"][1]) == 11


def test_the_package_defines_no_autograd_function_for_nfm():
    from deep_recommenders_amd import layers
    from deep_recommenders_amd.keras.models.ranking import nfm
    for mod in (nfm,):
        src = inspect.getsource(mod)
        assert not re.search(r"class\s+\w+\(.*autograd\.Function", src)
        for _, obj in inspect.getmembers(mod, inspect.isclass):
            assert not issubclass(obj, torch.autograd.Function)
    for src in (inspect.getsource(layers), inspect.getsource(ops)):
        for m in re.finditer(r"class\s+(\w+)\(.*autograd\.Function", src):
            assert "bi" not in m.group(1).lower().split("_") and "nfm" not in m.group(1).lower(), m.group(1)
