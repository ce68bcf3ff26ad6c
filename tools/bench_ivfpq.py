"""The IVF-PQ index (FaissIVFPQ: dr_pq_encode / dr_ivfpq_scan / dr_rerank_topk) against IVF-Flat (Faiss) on the same nlist / nprobe and
against BruteForce, all in ONE process per cell, alternating.

  python tools/bench_ivfpq.py [--rounds 5] [--iters 1 (the least per window; raised to fill ~50 ms)] [--cells n20_d64,...]
                              [--limit 900 (seconds per cell)] [--log profiles/ivfpq_bench.log]

Cells: N = 2^20 and 2^22 candidates at D 64 and 128 -- unit vectors around 4 096 random centres (x = c + 0.5 g, g ~ N(0, I / D),
normalised; the queries are drawn the same way) -- nlist 1024, nprobe 16 and 64, Bq 8192, k 100.  Per cell: BruteForce (the recall
yardstick), Faiss (IVF-Flat, the time yardstick), FaissIVFPQ with m = D / 4 and m = D / 8, each without refine and with refine = 4
(k * 4 > 128, so the scan hands its 128 best to the re-ranking), and the ADC scan alone (dr_ivfpq_scan on ready-made probes), whose
code bytes per second -- the 64-vector blocks of every probed list times m bytes, per query -- are set against the copy ceiling
(dr_copy_nt, read + write) measured in the same call.  The refining index shares the trained state of the plain one (the codebooks
are not bit-reproducible from build to build).  Every cell runs in a fresh child process under its own time limit, and the first
failing cell stops the run.  Device events; every variant is warmed up; the variants alternate inside every round; median, min and
the spread (max - min) / median are printed with every figure."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ffm import measure  # noqa: E402

NLIST, BQ, K, CENTRES, REFINE = 1024, 8192, 100, 4096, 4
NPROBES = (16, 64)
# cell -> (N, D)
CELLS = {"n%d_d%d" % (lg, D): (1 << lg, D) for lg in (20, 22) for D in (64, 128)}


def _unit_rows(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def _clustered(n, centres, gen):
    import torch
    D = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), device="cuda", generator=gen)
    g = torch.empty((n, D), device="cuda").normal_(0, 1.0 / D ** 0.5, generator=gen)
    return _unit_rows(centres[pick] + 0.5 * g).contiguous()


def _nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors if t is not None))


def _recall(got, want, k):
    """mean share of want[:, :k] found in got[:, :k]"""
    hit = (got[:, :k, None] == want[:, None, :k]).any(-1)
    return round(float(hit.float().mean()), 4)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t0, 3)


def bench_cell(name, rounds, iters):
    import torch
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.retrieval import factorized_top_k as ftk
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivfpq needs a GPU: a timing taken elsewhere says nothing")
    torch.cuda.set_device(0)
    N, D = CELLS[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    centres = _unit_rows(torch.empty((CENTRES, D), device="cuda").normal_(0, 1.0, generator=gen))
    cand = _clustered(N, centres, gen)
    q = _clustered(BQ, centres, gen)

    brute, t_brute = _timed(lambda: ftk.BruteForce(k=K).index(cand))
    flat, t_flat = _timed(lambda: ftk.Faiss(k=K, nlist=NLIST, nprobe=NPROBES[0]).index(cand))
    build = {"brute_force_s": t_brute, "ivf_flat_s": t_flat}
    index_bytes = {"brute_force": _nbytes(cand), "ivf_flat": _nbytes(flat._centroids, flat._packed, flat._packed_ids, flat._blk_off)}
    pqs = {}
    for m in (D // 4, D // 8):
        plain, t = _timed(lambda: ftk.FaissIVFPQ(k=K, nlist=NLIST, nprobe=NPROBES[0], m=m).index(cand))
        refined = ftk.FaissIVFPQ(k=K, nlist=NLIST, nprobe=NPROBES[0], m=m, refine=REFINE)
        for key, value in plain.state_dict().items():
            setattr(refined, key, value)                                        # the same trained state, plus the vectors
        refined._vectors = cand
        pqs[m] = (plain, refined)
        build["ivfpq_m%d_s" % m] = t
        index_bytes["ivfpq_m%d" % m] = _nbytes(plain._centroids, plain._codebooks, plain._packed_codes, plain._packed_rows, plain._blk_off)
        index_bytes["ivfpq_m%d_refine" % m] = index_bytes["ivfpq_m%d" % m] + _nbytes(cand)

    def with_nprobe(index, nprobe):
        def run():
            index._nprobe = nprobe
            return index(q)
        return run

    variants = {"brute_force": lambda: brute(q)}
    scans = {}
    for nprobe in NPROBES:
        variants["ivf_flat_np%d" % nprobe] = with_nprobe(flat, nprobe)
        for m, (plain, refined) in pqs.items():
            variants["ivfpq_m%d_np%d" % (m, nprobe)] = with_nprobe(plain, nprobe)
            variants["ivfpq_m%d_np%d_refine%d" % (m, nprobe, REFINE)] = with_nprobe(refined, nprobe)
            ps, probes = ops.topk_mips(q, plain._centroids, nprobe)
            blocks = (plain._blk_off[1:] - plain._blk_off[:-1])[probes].sum()
            scans["ivfpq_m%d_np%d_scan_only" % (m, nprobe)] = float(blocks.item()) * 64 * m
            variants["ivfpq_m%d_np%d_scan_only" % (m, nprobe)] = (
                lambda plain=plain, ps=ps, probes=probes: ops.ivfpq_scan(q, probes, ps, plain._blk_off, plain._packed_codes,
                                                                         plain._packed_rows, plain._codebooks, K))
    src = torch.empty(64 * 2 ** 20, device="cuda")                              # 256 MiB, read + write
    dst = torch.empty_like(src)
    variants["copy_nt"] = lambda: ops.copy_nt(src, dst)

    _, want = brute(q)
    recall = {}
    for n, fn in variants.items():
        if n.startswith("ivf") and not n.endswith("scan_only"):
            _, got = fn()
            recall[n] = {"recall@10": _recall(got, want, 10), "recall@100": _recall(got, want, 100)}
    res, reps = measure(variants, rounds, iters)
    med = lambda n: res[n]["median_ms"]                                                     # noqa: E731
    ceiling = 2.0 * src.numel() * 4 / (med("copy_nt") * 1e-3)
    scan = {n: {"code_GB_per_batch": round(b / 1e9, 3), "code_GBps": round(b / (med(n) * 1e-3) / 1e9, 1),
                "frac_of_copy_ceiling": round(b / (med(n) * 1e-3) / ceiling, 4)} for n, b in scans.items()}
    vs_flat = {n: round(med("ivf_flat_np%s" % n.split("_np")[1].split("_")[0]) / med(n), 3) for n in variants
               if n.startswith("ivfpq") and not n.endswith("scan_only")}
    out = {"shape": {"N": N, "D": D, "nlist": NLIST, "Bq": BQ, "k": K, "centres": CENTRES}, "iters_per_window": reps,
           "build": build, "index_MB": {n: round(b / 2 ** 20, 1) for n, b in index_bytes.items()}, "recall_vs_brute_force": recall,
           **res, "copy_ceiling_GBps": round(ceiling / 1e9, 1), "adc_scan": scan, "speedup_vs_ivf_flat_same_nprobe": vs_flat}
    print("%s: %s" % (name, json.dumps(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--limit", type=float, default=900.0, help="time limit of one cell, seconds")
    ap.add_argument("--log", default=None, help="also append the per-cell lines to this file")
    ap.add_argument("--cell", default=None, help="(internal) run this one cell in this process")
    a = ap.parse_args()
    if a.cell is not None:
        bench_cell(a.cell, a.rounds, a.iters)
        return
    for name in a.cells.split(","):
        if name not in CELLS:
            raise SystemExit("unknown cell %r; known: %s" % (name, ", ".join(CELLS)))
    for name in a.cells.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", name, "--rounds", str(a.rounds), "--iters", str(a.iters)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit, text=True)
        except subprocess.TimeoutExpired as e:
            print(e.stdout or "", flush=True)
            raise SystemExit("cell %s did not finish within %.0f s: stopping" % (name, a.limit))
        print(p.stdout, end="", flush=True)
        if p.returncode != 0:
            raise SystemExit("cell %s failed with exit status %d: stopping" % (name, p.returncode))
        if a.log:
            with open(a.log, "a") as log:
                log.writelines(line + "\n" for line in p.stdout.splitlines() if line.startswith(name + ": "))


if __name__ == "__main__":
    main()
