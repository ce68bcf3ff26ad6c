"""The BERT kernels against their fp32 torch compositions, ONE process, every variant of a section alternating inside every round,
with the copy ceiling (dr_copy_nt) measured in the same call:

  gelu    dr_gelu_fwd / dr_gelu_bwd                vs  F.gelu and its autograd backward                      [M, N] = [4096, 3072]
  embed   dr_bert_embed_fwd / _bwd                 vs  F.embedding x 3 + F.layer_norm + F.dropout (autograd)  B 32, L 128, D 768, V 30 522
  ce      dr_softmax_ce_ids (loss + gradient, in place)
                                                   vs  dr_softmax_ce_rows + _bwd on a dense one-hot [M, V] label matrix
                                                   vs  F.cross_entropy forward + backward on the logits         M 640, V 30 522
          and its share of the copy ceiling over its algorithmic bytes 2 M C 4 (the logits once in, once out)
  vocab   layers.vocab_cross_entropy, chunked      vs  the unchunked composition matmul + F.cross_entropy + autograd: time and the PEAK
          of torch's allocator                                                                         M 4096, D 768, V 30 522
  step    one BertPretraining.pretrain_step at B 32, L 128, base sizes (12 layers, D 768, H 12, F 3072), V 30 522, P 20

  python tools/bench_bert.py [--rounds 7] [--iters 3] [--sections gelu,embed,ce,vocab,step] [--log profiles/bert_bench.log]

Device events; every variant is warmed up; median, min and the spread (max - min) / median are printed with every figure.  A variant
wins only when its window lies outside the other's spread."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure, peak_mb                                            # noqa: E402  (the shared measuring loop)

V, D, H, F_, LAYERS, B, LN, P = 30522, 768, 12, 3072, 12, 32, 128, 20


def _finish(name, res, reps, extra, pairs):
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    wins = lambda a, b: bool(med(a) * (1 + res[a]["spread"]) < med(b) * (1 - res[b]["spread"]))   # noqa: E731
    line = {"iters_per_window": reps, **extra, **res}
    for mine, other in pairs:
        line["%s_speedup_vs_%s" % (mine, other)] = round(med(other) / med(mine), 3)
        line["%s_wins_vs_%s" % (mine, other)] = wins(mine, other)
    return "%s: %s" % (name, json.dumps(line))


def _ceiling(torch, ops, nbytes):
    src = torch.empty(max(4, int(nbytes // 8) // 4 * 4), device="cuda")
    dst = torch.empty_like(src)
    return (lambda: ops.copy_nt(src, dst)), 2.0 * src.numel() * 4


def bench_gelu(torch, ops, Fn, rounds, iters):
    M, N = 4096, F_
    z = torch.randn(M, N, device="cuda")
    dy = torch.randn(M, N, device="cuda")
    leaf = z.clone().requires_grad_(True)
    buf = torch.empty_like(dy)

    def torch_fwd():
        with torch.no_grad():
            return Fn.gelu(z)

    def torch_fwd_bwd():
        leaf.grad = None
        Fn.gelu(leaf).backward(dy)
        return leaf.grad

    def hip_fwd():
        return ops.gelu_fwd(z)

    def hip_fwd_bwd():
        h = ops.gelu_fwd(z)
        buf.copy_(dy)                               # the in-place backward owns its gradient buffer, as inside _MlpFn
        return h, ops.gelu_bwd_(z, buf)
    copy, copied = _ceiling(torch, ops, 8.0 * M * N)
    diff = float((hip_fwd() - torch_fwd()).abs().max())
    res, reps = measure({"torch_fwd": torch_fwd, "hip_fwd": hip_fwd, "torch_fwd_bwd": torch_fwd_bwd, "hip_fwd_bwd": hip_fwd_bwd,
                         "copy_nt": copy}, rounds, iters)
    ceiling = copied / (res["copy_nt"]["median_ms"] * 1e-3)
    extra = {"shape": [M, N], "max_abs_diff_fwd": diff, "copy_ceiling_GBps": round(ceiling / 1e9, 1),
             "hip_fwd_frac_of_copy_ceiling": round(8.0 * M * N / (res["hip_fwd"]["median_ms"] * 1e-3) / ceiling, 4)}
    return _finish("gelu", res, reps, extra, [("hip_fwd", "torch_fwd"), ("hip_fwd_bwd", "torch_fwd_bwd")])


def bench_embed(torch, ops, Fn, rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(1)
    tok = torch.randn(V, D, device="cuda", generator=gen) * 0.02
    pos = torch.randn(512, D, device="cuda", generator=gen) * 0.02
    seg = torch.randn(2, D, device="cuda", generator=gen) * 0.02
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    ids = torch.randint(0, V, (B, LN), device="cuda", generator=gen)
    sg = torch.randint(0, 2, (B, LN), device="cuda", generator=gen)
    d_out = torch.randn(B, LN, D, device="cuda", generator=gen)
    leaves = [t.clone().requires_grad_(True) for t in (tok, pos, seg, gamma, beta)]
    lpos = torch.arange(LN, device="cuda")
    d_tok = torch.zeros_like(tok)

    def compose(t, p, s, g, b, rate):
        x = Fn.embedding(ids, t) + Fn.embedding(lpos, p)[None] + Fn.embedding(sg, s)
        return Fn.dropout(Fn.layer_norm(x, (D,), g, b, eps=1e-12), rate)

    def torch_fwd():
        with torch.no_grad():
            return compose(tok, pos, seg, gamma, beta, 0.1)

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        compose(*leaves, 0.1).backward(d_out)
        return leaves[0].grad

    def hip_fwd():
        return ops.bert_embed_fwd(ids, sg, tok, pos, seg, gamma, beta, 1e-12, 0.1, 7)

    def hip_fwd_bwd():
        out, stats = ops.bert_embed_fwd(ids, sg, tok, pos, seg, gamma, beta, 1e-12, 0.1, 7)
        d_tok.zero_()
        return ops.bert_embed_bwd(ids, sg, tok, pos, seg, gamma, stats, d_out, d_tok, 0.1, 7)
    with torch.no_grad():
        diff = float((ops.bert_embed_fwd(ids, sg, tok, pos, seg, gamma, beta, 1e-12, 0.0, 7)[0] - compose(tok, pos, seg, gamma, beta, 0.0)).abs().max())
    res, reps = measure({"torch_fwd": torch_fwd, "hip_fwd": hip_fwd, "torch_fwd_bwd": torch_fwd_bwd, "hip_fwd_bwd": hip_fwd_bwd}, rounds, iters)
    extra = {"shape": {"B": B, "L": LN, "D": D, "V": V}, "max_abs_diff_fwd_rate0": diff,
             "peak_MB": {"torch_fwd_bwd": peak_mb(torch_fwd_bwd), "hip_fwd_bwd": peak_mb(hip_fwd_bwd)}}
    return _finish("embed", res, reps, extra, [("hip_fwd", "torch_fwd"), ("hip_fwd_bwd", "torch_fwd_bwd")])


def bench_ce(torch, ops, Fn, rounds, iters):
    M, C = B * P, V
    gen = torch.Generator(device="cuda").manual_seed(2)
    logits = torch.randn(M, C + 2, device="cuda", generator=gen)[:, :C]               # pitch 30 524, as vocab_cross_entropy's buffer
    dense = logits.contiguous()
    labels = torch.randint(0, C, (M,), device="cuda", generator=gen)
    onehot = torch.zeros(M, C, device="cuda").scatter_(1, labels[:, None], 1.0)
    w = torch.full((M,), 1.0 / M, device="cuda")
    work = torch.empty(M, C + 2, device="cuda")[:, :C]
    leaf = dense.clone().requires_grad_(True)

    def ids_kernel():
        work.copy_(logits)                          # in place: every call needs fresh logits; the copy is timed on its own below
        return ops.softmax_ce_ids(work, labels, None, w)

    def refill():
        work.copy_(logits)

    def rows_onehot():
        return ops.softmax_ce_rows(dense, onehot, 1.0, w), ops.softmax_ce_rows_bwd(dense, onehot, 1.0, w, 1.0)

    def torch_ce():
        leaf.grad = None
        Fn.cross_entropy(leaf, labels, reduction="mean").backward()
        return leaf.grad
    copy, copied = _ceiling(torch, ops, 2.0 * M * C * 4)
    g_ref = torch_ce().clone()
    ids_kernel()
    diff = float((work - g_ref).abs().max() / g_ref.abs().max())
    res, reps = measure({"softmax_ce_ids_with_refill": ids_kernel, "refill_copy": refill, "softmax_ce_rows_onehot": rows_onehot,
                         "torch_cross_entropy": torch_ce, "copy_nt": copy}, rounds, iters)
    net = res["softmax_ce_ids_with_refill"]["median_ms"] - res["refill_copy"]["median_ms"]
    ceiling = copied / (res["copy_nt"]["median_ms"] * 1e-3)
    extra = {"shape": {"M": M, "C": C}, "max_rel_diff_grad_vs_torch": diff, "softmax_ce_ids_net_ms": round(net, 4),
             "copy_ceiling_GBps": round(ceiling / 1e9, 1), "algorithmic_bytes": 2 * M * C * 4,
             "softmax_ce_ids_frac_of_copy_ceiling": round(2.0 * M * C * 4 / (max(net, 1e-6) * 1e-3) / ceiling, 4),
             "softmax_ce_ids_net_speedup_vs_rows_onehot": round(res["softmax_ce_rows_onehot"]["median_ms"] / max(net, 1e-6), 3),
             "softmax_ce_ids_net_speedup_vs_torch": round(res["torch_cross_entropy"]["median_ms"] / max(net, 1e-6), 3),
             "onehot_MB": round(M * C * 4 / 2 ** 20, 1)}
    return _finish("ce", res, reps, extra, [])


def bench_vocab(torch, ops, Fn, rounds, iters):
    from deep_recommenders_amd import layers as L
    M = B * LN
    gen = torch.Generator(device="cuda").manual_seed(3)
    t = torch.randn(M, D, device="cuda", generator=gen)
    table = torch.randn(V, D, device="cuda", generator=gen) * 0.02
    bias = torch.zeros(V, device="cuda")
    labels = torch.randint(0, V, (M,), device="cuda", generator=gen)
    d_table, d_bias = torch.zeros_like(table), torch.zeros_like(bias)
    leaves = [x.clone().requires_grad_(True) for x in (t, table, bias)]

    def chunked(chunk_rows=None):
        d_table.zero_(), d_bias.zero_()
        return L.vocab_cross_entropy(t, table, bias, labels, row_scale=1.0 / M, d_table=d_table, d_bias=d_bias, chunk_rows=chunk_rows)

    def unchunked():
        for x in leaves:
            x.grad = None
        Fn.cross_entropy(leaves[0] @ leaves[1].t() + leaves[2], labels, reduction="mean").backward()
        return leaves[0].grad
    want = unchunked().clone()
    diff = float((chunked()[1] - want).abs().max() / want.abs().max())
    peaks = {"vocab_cross_entropy_default": peak_mb(chunked), "vocab_cross_entropy_chunk_512": peak_mb(lambda: chunked(512)),
             "unchunked_torch": peak_mb(unchunked)}
    res, reps = measure({"vocab_cross_entropy": chunked, "unchunked_torch": unchunked}, rounds, iters)
    extra = {"shape": {"M": M, "D": D, "V": V}, "max_rel_diff_d_t_vs_torch": diff, "peak_MB": peaks,
             "logits_MB": round(M * V * 4 / 2 ** 20, 1)}
    return _finish("vocab", res, reps, extra, [("vocab_cross_entropy", "unchunked_torch")])


def bench_step(torch, ops, Fn, rounds, iters):
    from deep_recommenders_amd import optim
    from deep_recommenders_amd.keras.models.nlp import BERT, BertPretraining
    head = BertPretraining(BERT(V, D, LAYERS, H, F_, seed=1))
    opt = optim.Adam(head.parameters(), lr=1e-4)
    gen = torch.Generator(device="cuda").manual_seed(4)
    ids = torch.randint(5, V, (B, LN), device="cuda", generator=gen)
    ids[:, 0] = 2
    seg = (torch.arange(LN, device="cuda")[None, :] >= LN // 2).to(torch.int64).expand(B, LN).contiguous()
    nsp = torch.randint(0, 2, (B,), device="cuda", generator=gen)

    def step():
        return head.pretrain_step(ids, seg, nsp, opt, max_predictions=P)
    first = [float(x) for x in step()]
    res, reps = measure({"pretrain_step": step}, rounds, iters)
    extra = {"shape": {"B": B, "L": LN, "layers": LAYERS, "D": D, "H": H, "F": F_, "V": V, "P": P}, "first_losses": first,
             "peak_MB": peak_mb(step), "tokens_per_s": round(B * LN / (res["pretrain_step"]["median_ms"] * 1e-3))}
    return _finish("step", res, reps, extra, [])


SECTIONS = {"gelu": bench_gelu, "embed": bench_embed, "ce": bench_ce, "vocab": bench_vocab, "step": bench_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--log", default=None, help="also append the per-section lines to this file")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as Fn
    from deep_recommenders_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    for name in a.sections.split(","):
        if name not in SECTIONS:
            raise SystemExit("unknown section %r; known: %s" % (name, ", ".join(SECTIONS)))
    for name in a.sections.split(","):
        line = SECTIONS[name](torch, ops, Fn, a.rounds, a.iters)
        print(line, flush=True)
        if a.log:
            with open(a.log, "a") as log:
                log.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
