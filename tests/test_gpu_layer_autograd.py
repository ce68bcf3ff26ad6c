"""Every autograd Function of the package (deep_recommenders_amd/layers.py, losses.py and the model files that define their own),
called directly, with the incoming gradient in every layout torch produces.  The table, the recipes, the probe and the references are in tests/layer_autograd_cases.py (checked on the CPU by
tests/test_layer_autograd_cpu.py); this file drives them on the device.

Each case compares the forward value and every gradient with a float64 reference differentiated by torch's autograd, under the
bound the layer's kernels already have in their own test files (named next to each entry of the table).  A probe directly after
every output asserts the strides the gradient arrived with, so a case cannot silently stop testing its layout.

Held to bit-equality across layouts (the same gradient values, materialised contiguously, give the same bits): every entry whose
backward runs in a fixed order -- the CSR and the dense aggregate, softmax, attention, add-layer-norm, token embedding, tied
projection, Dice, DIN pooling, CIN, dot interaction, AFM, PNN, GRU, sequence attention, FFM interaction, and the element-wise ones.
Held to the float64 bound only, because partial sums meet in fp32 atomics whose order changes from run to run: mlp, cross and
cross_low_rank and the retrieval Functions (linear_bwd_dw without a workspace), the embedding backward without a plan (EmbeddingSlab,
_LinFieldsFn, ffm_gather, sgns_loss and eges_loss through K4) and DIEN's item rows (dr_rows_scatter_add).  sgns_loss and eges_loss
with plans, the losses, the CIN layer, the row dot product, DIN's concat and the two multi-task Functions (every dW of theirs takes
a workspace) run in a fixed order and are held to bit-equality.

Not in the table: `activation` with act 0 (it returns its input; there is no Function), `afm_pooling`'s attention output and
EmbeddingSlab's sum_x (marked non-differentiable: no gradient can be sent into them), `aggregate`'s adjacency (a graph input), and the
in-place SGD mode (`sparse_lr`) of sgns_loss and eges_loss, which returns no gradient (tests/test_gpu_sgns.py and test_gpu_eges.py
check the tables it leaves).  tests/test_layer_autograd_cpu.py reads the package with `ast` and fails when a Function has no entry.

A float64 or float16 gradient handed to torch.autograd.backward does not raise in this torch: the engine casts it to the output's
dtype before the first backward runs.  test_foreign_dtype_gradient_is_cast_before_the_layer pins that no kernel sees another dtype."""
import importlib
import itertools

import pytest
import torch

import layer_autograd_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(name, B) for name in C.ENTRIES for B in C.BATCHES]
IDS = ["%s-B%d" % c for c in CASES]
REPORT = {}


def _usages(n_out):
    """which outputs are used: all of them first, then every other non-empty subset (each output alone, every pair, ...)"""
    return [u for u in itertools.product((True, False), repeat=n_out) if any(u)]


def _recipes(res_dims, name, used):
    return [C.recipe_named(d, name, default="base") if u else None for d, u in zip(res_dims, used)]


def _dims(entry, case):
    leaves, shown = C.leaves_for(case, entry.diff, torch.float32, DEV)
    with torch.no_grad():
        outs = entry.call(shown)
    outs = outs if isinstance(outs, tuple) else (outs,)
    return [o.dim() for o in outs]


def _same_grads(entry, a, b, what):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, "%s %s: %s" % (entry.name, what, k)
        else:
            assert C.bits_equal(a[k], b[k]), "%s %s: the gradient of %s changed bits" % (entry.name, what, k)


def _untouched(res, what):
    for seen in res["seen"]:
        for s in seen:
            assert C.bits_equal(s["grad"].contiguous(), s["before"].contiguous()), "%s: the incoming gradient was written to" % what


@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_every_gradient_layout(name, B):
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    report = REPORT.setdefault(name, {})
    first = True
    for used in _usages(len(dims)):
        names = [n for n in C.RECIPE_NAMES if any(r[0] == n for d, u in zip(dims, used) if u for r in C.RECIPES[d])]
        for rname in (names if all(used) else ["base", "sum"]):
            recipes = _recipes(dims, rname, used)
            res = C.run_layer(entry, case, DEV, recipes, seed=B)
            # (an output marked non-differentiable, afm_pooling's attention, takes no probe: nothing can be sent into it)
            assert all(len(s) == 1 for s, G in zip(res["seen"], res["G"]) if G is not None), "a used output's probe saw one gradient"
            C.check_against_reference(entry, case, res, forward=first, report=report)
            _untouched(res, "%s %s" % (name, rname))
            first = False
            if entry.bit_equal and rname != "base":
                dense = C.run_layer(entry, case, DEV, [None if r is None else C.materialised(r) for r in recipes], seed=B)
                _same_grads(entry, res["grads"], dense["grads"], "layout %s against the same values made contiguous" % rname)
    print("%s B=%d: largest err / bound %s" % (name, B, ", ".join("%s %.3f" % kv for kv in sorted(report.items()))))


@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_output_consumed_twice_and_backward_twice(name, B):
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    res = C.run_layer(entry, case, DEV, [C.TWICE if d > 0 else C.RECIPES[0][0] for d in dims], seed=B, times=2)
    C.check_against_reference(entry, case, res, forward=False, report=REPORT.setdefault(name, {}))
    _untouched(res, name)
    if entry.bit_equal:
        _same_grads(entry, res["runs"][0], res["runs"][1], "backward(retain_graph=True) twice")
    else:                                                  # fp32 atomics: the second run is held to the same float64 bound
        C.check_against_reference(entry, case, dict(res, grads=res["runs"][1]), forward=False)
    # a gradient that is ours, handed over by hand: bit-unchanged afterwards (_ActFn, _MlpFn and act_bwd_ work in place)
    mine = C.run_layer(entry, case, DEV, [C.recipe_named(d, "hand", default="base") for d in dims], seed=B, times=2)
    _untouched(mine, name)


def _watch_backwards(monkeypatch, returned):
    """Wraps the backward of every Function of the package (every class the inventory of tests/layer_autograd_cases.py finds): what a
    backward RETURNS is what is checked (autograd drops, without a word, a tensor returned for an input that needs none, so a leaf's
    .grad cannot show it).  Slot i must be None when needs_input_grad[i] is False -- a frozen input, or an argument that is no
    tensor.  The Functions whose gradients all come out of one fused kernel (DIN pooling, CIN, AFM, PNN, GRU, attention,
    add-layer-norm, Dice, the cross combine, DIN's concat, the losses) still compute an unneeded gradient inside that launch;
    layers._needed_only drops it before it is returned.  The GEMM-built ones (mlp, cross, tied projection, the aggregates, the
    retrieval Functions) and DIEN's row dot product do not launch the kernel of a gradient nobody needs."""
    for module, cls_name in C.package_functions():
        cls = getattr(importlib.import_module(module), cls_name)

        def watched(ctx, *grads, _real=cls.backward, _name=cls.__name__):
            out = _real(ctx, *grads)
            out = out if isinstance(out, tuple) else (out,)
            assert len(out) == len(ctx.needs_input_grad), _name
            for i, (g, need) in enumerate(zip(out, ctx.needs_input_grad)):
                assert need or g is None, "%s.backward returned a gradient in slot %d, which needs none" % (_name, i)
            returned.append((_name, tuple(g is not None for g in out), tuple(ctx.needs_input_grad)))
            return out
        monkeypatch.setattr(cls, "backward", staticmethod(watched))


@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_each_input_frozen_in_turn(name, B, monkeypatch):
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    recipes = [C.recipe_named(d, "base") for d in dims]
    returned = []
    _watch_backwards(monkeypatch, returned)
    full = C.run_layer(entry, case, DEV, recipes, seed=B)
    assert returned, "no backward of the package ran under the watch"
    for frozen in [k for k in entry.diff if case.get(k) is not None]:
        del returned[:]
        res = C.run_layer(entry, case, DEV, recipes, frozen=(frozen,), seed=B)
        if any(l.requires_grad for l in res["leaves"].values()):
            assert returned and any(not all(needs) for _, _, needs in returned), "%s: freezing %s reached no backward" % (name, frozen)
        assert res["grads"][frozen] is None, "%s: the frozen %s received a gradient" % (name, frozen)
        if not any(l.requires_grad for l in res["leaves"].values()):
            continue
        C.check_against_reference(entry, case, res, forward=False)
        if entry.bit_equal:
            _same_grads(entry, {k: v for k, v in res["grads"].items() if k != frozen},
                        {k: v for k, v in full["grads"].items() if k != frozen}, "with %s frozen" % frozen)


PRESENTED = [(n, B) for n, B in CASES if C.ENTRIES[n].present]


@pytest.mark.parametrize("name,B", PRESENTED, ids=["%s-B%d" % c for c in PRESENTED])
def test_inputs_handed_over_as_views(name, B):
    """a column slice of a padded buffer, a transposed weight, an expanded bias: the gradient lands in the leaf behind the view, in
    the leaf's shape"""
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    for rname in ("base", "sum0" if 2 in dims else "sum"):
        res = C.run_layer(entry, case, DEV, [C.recipe_named(d, rname, default="base") for d in dims], present=entry.present, seed=B)
        for k, leaf in res["leaves"].items():
            if leaf.requires_grad:
                assert res["grads"][k] is not None and res["grads"][k].shape == leaf.shape and res["grads"][k].dtype == torch.float32
        C.check_against_reference(entry, case, res, present=entry.present, report=REPORT.setdefault(name, {}))


@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_foreign_dtype_gradient_is_cast_before_the_layer(name, B):
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    base = C.run_layer(entry, case, DEV, [C.materialised(C.recipe_named(d, "base")) for d in dims], seed=B)
    for dtype in (torch.float64, torch.float16):
        def foreign(rec):
            return (rec[0], "hand", lambda a, s, v=rec[3]: v(s, a).to(dtype), lambda s, a, v=rec[3]: v(s, a).to(dtype).float(), lambda s: None)
        res = C.run_layer(entry, case, DEV, [foreign(C.recipe_named(d, "base")) for d in dims], seed=B)
        assert all(s["dtype"] == torch.float32 for seen in res["seen"] for s in seen), "a %s gradient reached the layer" % dtype
        if dtype == torch.float64 and entry.bit_equal:     # float32 values held in float64: the cast changes nothing
            _same_grads(entry, res["grads"], base["grads"], "float64 gradient")
        C.check_against_reference(entry, case, res, forward=False)


SPIED = [(n, B) for n, B in CASES if C.ENTRIES[n].spy]


@pytest.mark.parametrize("name,B", SPIED, ids=["%s-B%d" % c for c in SPIED])
def test_baseline_gradient_reaches_ops_untouched(name, B, monkeypatch):
    """No copy on the path the models take: under the baseline layout (contiguous, 16-byte aligned) the tensor the ops wrapper
    receives has the incoming gradient's data_ptr.  dot_interaction's kernel reads rows at a pitch that is a multiple of 4, as it did
    before: there a width that is no multiple of 4 reaches ops as ONE padded copy when there are several rows, and untouched
    (one row has no pitch) at batch 1."""
    from deep_recommenders_amd import ops
    entry = C.ENTRIES[name]
    case = entry.build(B)
    dims = _dims(entry, case)
    fn_name, index = entry.spy
    real, got = getattr(ops, fn_name), []

    def spy(*args, **kw):
        if args[index] is not None:
            got.append((args[index].data_ptr(), tuple(args[index].shape), tuple(args[index].stride())))
        return real(*args, **kw)
    monkeypatch.setattr(ops, fn_name, spy)
    res = C.run_layer(entry, case, DEV, [C.recipe_named(d, "base") for d in dims], seed=B)
    seen = res["seen"][0][0]
    shape = tuple(res["outs"][0].shape)
    if name.startswith("dot_interaction") and shape[-1] % 4 != 0 and B > 1:
        (ptr, shp, strides), = got                           # the backward's one call
        assert ptr != seen["ptr"] and shp == shape and strides == (C.pad4(shape[-1]), 1), (name, got)
        return
    assert seen["ptr"] in [g[0] for g in got], "%s: the gradient was copied before %s" % (name, fn_name)


def test_zz_report():
    """the largest err / bound measured per layer and quantity (forward out<k>, gradients d_<input>), for the commit message"""
    for name in sorted(REPORT):
        print("%-28s %s" % (name, "  ".join("%s %.3f" % kv for kv in sorted(REPORT[name].items()))))


# Largest err / bound read on an MI355X when this file was written, over every layout, usage and batch of an entry (out<k>: forward
# output k, d_<input>: that input's gradient).  dropout and ffm_interaction's d_rows are one fp32 rounding against a bound of one
# rounding; 0.000 is an exact copy or sum.
#   activation_sigmoid           d_x 0.026  out0 0.422
#   activation_tanh              d_x 0.103  out0 0.354
#   add_layer_norm_D1            d_a 0.000  d_b 0.000  d_beta 0.005  d_gamma 0.000  out0 0.000
#   add_layer_norm_D5            d_a 0.008  d_b 0.008  d_beta 0.085  d_gamma 0.014  out0 0.032
#   add_layer_norm_D6            d_a 0.007  d_beta 0.065  d_gamma 0.013  out0 0.044
#   add_residual                 d_out 0.000  d_x 0.000  out0 0.490
#   afm_pooling_F2               d_W 0.000  d_b 0.000  d_emb 0.007  d_h 0.000  out0 0.005
#   afm_pooling_F3               d_W 0.034  d_b 0.106  d_emb 0.030  d_h 0.059  out0 0.019
#   afm_pooling_with_attention   d_W 0.034  d_b 0.106  d_emb 0.030  d_h 0.059  out0 0.019  out1 0.002
#   aggregate_dense              d_X 0.004  out0 0.014
#   aggregate_sparse             d_X 0.010  out0 0.009
#   attention_H1                 d_k 0.000  d_q 0.000  d_v 0.000  out0 0.000
#   attention_H2                 d_k 0.008  d_q 0.004  d_v 0.023  out0 0.016
#   cin_pool_act0                d_W 0.005  d_bias 0.004  d_x 0.001  d_x0 0.002  out0 0.011  out1 0.005
#   cin_pool_act2                d_W 0.009  d_bias 0.016  d_x 0.004  d_x0 0.004  out0 0.002  out1 0.002
#   cin_stack_act0               d_W 0.004  d_W2 0.002  d_bias 0.002  d_bias2 0.004  d_x0 0.002  out0 0.000
#   cin_stack_act1               d_W 0.003  d_W2 0.002  d_bias 0.002  d_bias2 0.002  d_x0 0.002  out0 0.000
#   cross                        d_W 0.005  d_b 0.004  d_x 0.006  d_x0 0.003  out0 0.015
#   cross_low_rank               d_U 0.005  d_V 0.007  d_b 0.003  d_x 0.004  d_x0 0.004  out0 0.006
#   cross_low_rank_transposed    d_U 0.005  d_V 0.007  d_b 0.003  d_x 0.004  d_x0 0.004  out0 0.006
#   cross_transposed_W           d_W 0.005  d_b 0.004  d_x 0.006  d_x0 0.003  out0 0.015
#   dice_N1                      d_alpha 0.032  d_x 0.000  out0 0.011
#   dice_N5                      d_alpha 0.112  d_x 0.057  out0 0.034
#   din_interest_pooling_T1      d_W 0.086  d_b 0.176  d_b_out 0.343  d_keys 0.078  d_query 0.072  d_w_out 0.074  out0 0.041  out1 0.042
#   din_interest_pooling_T5      d_W 0.101  d_alpha 0.272  d_b 0.289  d_b_out 0.063  d_keys 0.087  d_query 0.115  d_w_out 0.122  out0 0.074  out1 0.054
#   dot_interaction_F1_dense     d_dense 0.286  d_emb 0.193  out0 0.329
#   dot_interaction_F2_nodense   d_emb 0.196  out0 0.255
#   dot_interaction_F3_dense     d_dense 0.257  d_emb 0.274  out0 0.250
#   dot_interaction_F7_dense     d_dense 0.173  d_emb 0.213  out0 0.383
#   dropout                      d_x 0.932  out0 0.922
#   embedding_slab               d_lin_bias 0.001  d_lin_w 0.015  d_table 0.006  out0 0.000  out1 0.135
#   ffm_gather_F2                d_lin_bias 0.001  d_lin_w 0.019  d_table 0.005  out0 0.229  out1 0.415
#   ffm_gather_F3                d_lin_bias 0.001  d_lin_w 0.005  d_table 0.005  out0 0.040  out1 0.288
#   ffm_interaction_F2           d_rows 0.982  out0 0.334
#   ffm_interaction_F3           d_rows 0.981  out0 0.043
#   fm_second_order              d_x 0.032  out0 0.018
#   gather_cols                  d_emb 0.000  out0 0.000
#   global_average_pooling_1d    d_x 0.007  out0 0.014
#   gru_sequence_T1              d_U 0.038  d_h0 0.024  d_xp 0.019  out0 0.014  out1 0.011
#   gru_sequence_T5              d_U 0.039  d_att 0.024  d_h0 0.026  d_xp 0.028  out0 0.013  out1 0.010
#   input_layer                  d_table 0.003  out0 0.000
#   l2_penalty                   d_w 0.488  out0 0.014
#   lin_fields                   d_lin_w 0.007  out0 0.000
#   mlp                          d_W0 0.005  d_W1 0.016  d_b0 0.008  d_b1 0.040  d_x 0.004  out0 0.005
#   mlp_sigmoid_top              d_W0 0.009  d_b0 0.007  d_x 0.010  out0 0.008
#   mlp_transposed_W             d_W0 0.005  d_W1 0.016  d_b0 0.008  d_b1 0.040  d_x 0.004  out0 0.006
#   pnn_outer_F1                 d_W 0.033  d_addend 0.000  d_emb 0.010  out0 0.007
#   pnn_outer_F3                 d_W 0.033  d_addend 0.000  d_emb 0.018  out0 0.028
#   sequence_attention_T1        d_hs 0.000  d_q 0.000  out0 0.000
#   sequence_attention_T5        d_hs 0.457  d_q 0.167  out0 0.031
#   softmax_rows                 d_x 0.082  out0 0.245
#   tied_projection              d_table 0.007  d_x 0.014  out0 0.008
#   tied_projection_transposed   d_table 0.007  d_x 0.014  out0 0.008
#   token_embedding              d_table 0.119  out0 0.126
#   token_embedding_dropout      d_table 0.134  out0 0.146
#
# The entries of the rest of the package (losses.py, sbcnm.py, xdeepfm.py, dien.py, din.py, the two multi-task Functions) and of
# sgns_loss / eges_loss, read on an MI355X when they were added.  row_dot's gradients are one correctly rounded multiply (dr_rows_scale)
# against a bound of one rounding, and so are the third block of din_concat_mode1 / mode2 and din_subtract / din_multiply forward (one
# subtraction or product, u |ref|); din_concat_mode0 and mean_squared_error's d_p at 0.000 are copies resp. far inside a 1e-4 bound.
#   binary_crossentropy         d_x 0.174  out0 0.013
#   categorical_crossentropy_logits  d_x 0.044  out0 0.002
#   categorical_crossentropy_logits_weighted  d_x 0.044  out0 0.001
#   categorical_crossentropy_prob  d_x 0.001  out0 0.006
#   categorical_crossentropy_prob_weighted  d_x 0.001  out0 0.007
#   cin_act0                    d_W 0.004  d_x 0.002  d_x0 0.001  out0 0.004
#   cin_act0_bias               d_W 0.004  d_bias 0.002  d_x 0.002  d_x0 0.001  out0 0.005
#   cin_act2                    d_W 0.004  d_x 0.003  d_x0 0.004  out0 0.002
#   cin_act2_bias               d_W 0.005  d_bias 0.034  d_x 0.005  d_x0 0.004  out0 0.002
#   din_concat_mode0            d_x 0.000  d_y 0.000  out0 0.000
#   din_concat_mode1            d_x 0.186  d_y 0.153  out0 0.971
#   din_concat_mode2            d_x 0.120  d_y 0.138  out0 0.962
#   din_multiply                d_x 0.174  d_y 0.192  out0 0.986
#   din_subtract                d_x 0.000  d_y 0.000  out0 0.971
#   eges_loss_att_P1_atomics    d_att 0.003  d_out_table 0.003  d_side_table 0.004  out0 0.010
#   eges_loss_att_P2_plans      d_att 0.003  d_out_table 0.004  d_side_table 0.003  out0 0.014
#   eges_loss_noatt_P1_plans    d_out_table 0.002  d_side_table 0.003  out0 0.010
#   eges_loss_noatt_P2_atomics  d_out_table 0.003  d_side_table 0.003  out0 0.011
#   esmm                        d_pCTR/dense/bias 0.001  d_pCTR/dense/kernel 0.001  d_pCTR/dense_1/bias 0.002  d_pCTR/dense_1/kernel 0.002
#                               d_pCVR/dense/bias 0.001  d_pCVR/dense/kernel 0.001  d_pCVR/dense_1/bias 0.001  d_pCVR/dense_1/kernel 0.001
#                               d_x 0.001  out0 0.001  out1 0.001  out2 0.001
#   explicit_softmax            d_c 0.002  d_q 0.004  out0 0.003
#   explicit_softmax_all        d_c 0.004  d_q 0.024  out0 0.001
#   hard_negative_softmax       d_c 0.002  d_q 0.003  out0 0.000
#   hard_negative_softmax_all   d_c 0.008  d_q 0.004  out0 0.000
#   inbatch_softmax             d_c 0.005  d_q 0.009  out0 0.000
#   inbatch_softmax_all         d_c 0.015  d_q 0.022  out0 0.002
#   item_rows_pitched           d_table 0.211  out0 0.000
#   item_rows_transposed        d_table 0.211  out0 0.000
#   log_loss                    d_x 0.208  out0 0.002
#   losses_sigmoid              d_x 0.029  out0 0.004
#   mean_squared_error_T1       d_p 0.000  out0 0.001
#   mean_squared_error_T3       d_p 0.000  out0 0.000
#   mmoe                        d_mixture_of_experts/dense/bias 0.001  d_mixture_of_experts/dense/kernel 0.001
#                               d_mixture_of_experts/dense_1/bias 0.001  d_mixture_of_experts/dense_1/kernel 0.001
#                               d_mixture_of_experts/dense_2/bias 0.001  d_mixture_of_experts/dense_2/kernel 0.001
#                               d_multi_gate/dense/kernel 0.001  d_multi_gate/dense_1/kernel 0.003  d_task0/dense/bias 0.003
#                               d_task0/dense/kernel 0.002  d_task0/dense_1/bias 0.004  d_task0/dense_1/kernel 0.002
#                               d_task1/dense/bias 0.001  d_task1/dense/kernel 0.001  d_task1/dense_1/bias 0.004
#                               d_task1/dense_1/kernel 0.001  d_x 0.001  out0 0.001  out1 0.002
#   retrieval_adjust            d_scores 0.000  out0 0.314
#   retrieval_adjust_ids        d_scores 0.000  out0 0.314
#   retrieval_scores            d_c 0.008  d_q 0.034  out0 0.127
#   retrieval_scores_transposed  d_c 0.008  d_q 0.034  out0 0.127
#   row_dot                     d_a 0.977  d_b 0.978  out0 0.277
#   sgns_loss_K0_keep_atomics   d_in_table 0.003  d_out_table 0.002  out0 0.008
#   sgns_loss_K0_skip_plans     d_in_table 0.003  d_out_table 0.002  out0 0.008
#   sgns_loss_K5_keep_plans     d_in_table 0.003  d_out_table 0.003  out0 0.009
#   sgns_loss_K5_skip_atomics   d_in_table 0.002  d_out_table 0.003  out0 0.009
#   sigmoid_cross_entropy       d_x 0.008  out0 0.003
