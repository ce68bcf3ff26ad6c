"""GPU tests of the IVF-PQ index (csrc/ivf_pq.hip, ops.pq_encode / ivfpq_scan / rerank_topk, FaissIVFPQ, EBR kind="ivfpq") against
the NumPy restatement tests/ivfpq_ref.py.  Integer grids are compared bit for bit, exact ties included; random inputs against bounds
derived from the fp32 arithmetic (ivfpq_ref.adc_bound / rerank_bound; u = 2^-24), with a COMPLETE check of every search result: every
returned score within its bound, the list sorted, and no candidate of the probed lists that was left out better than the k-th
returned one by more than the two bounds.  Every test prints its largest error / bound."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words_dev(words):
    return _dev(np.ascontiguousarray(words).view(np.int32))


# ---- pq_encode -----------------------------------------------------------------------------------------------------------------------
ENCODE_SHAPES = [(8, 4), (32, 8), (96, 8), (64, 16), (256, 4), (64, 64)]


@pytest.mark.parametrize("with_centroids", [True, False])
@pytest.mark.parametrize("D,m", ENCODE_SHAPES)
def test_pq_encode_integer_grids_bit_for_bit(D, m, with_centroids):
    """|v| <= 8 everywhere: every difference, square and sum is an integer below 2^24, so the fp32 distances are exact and the codes
    must equal the reference's -- with duplicated codewords and vectors placed ON them, so that exact ties occur and the lower code
    must win; one case carries assignments outside [0, nlist)."""
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(D * 100 + m)
    N, nlist, dsub = 193, 5, D // m
    cb = rng.integers(-8, 9, size=(m, R.KSUB, dsub)).astype(np.float32)
    cb[:, 200] = cb[:, 7]                                                        # duplicates: 7 must win over 200, 0 over 255
    cb[:, 255] = cb[:, 0]
    cen = rng.integers(-8, 9, size=(nlist, D)).astype(np.float32)
    assign = rng.integers(0, nlist, size=N)
    res = rng.integers(-8, 9, size=(N, D)).astype(np.float32)
    res[:40] = np.concatenate([cb[j, rng.choice([7, 200, 0, 255, 31], size=40)] for j in range(m)], axis=1)      # on a codeword
    if with_centroids:
        x = res + cen[assign]
        if (D, m) == (32, 8):
            assign[[3, 50, 192]] = [-1, nlist, 2 ** 40]
        got = ops.pq_encode(_dev(x), _dev(cb), _dev(assign), _dev(cen))
        want = R.encode(x, cb, assign, cen)
    else:
        x = res
        got = ops.pq_encode(_dev(x), _dev(cb))
        want = R.encode(x, cb)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, m // 4)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)
    codes = R.code_bytes(want, m)
    assert not np.isin(codes, [200, 255]).any()                                 # the duplicates never win
    keep = np.ones(N, dtype=bool)
    if with_centroids and (D, m) == (32, 8):
        keep[[3, 50, 192]] = False
    for j in range(m):                                                           # a vector placed on a codeword is at distance 0 of its code
        on = np.flatnonzero(keep[:40])
        np.testing.assert_array_equal(cb[j, codes[on, j]], res[on, j * dsub:(j + 1) * dsub])
    if with_centroids and (D, m) == (32, 8):
        assert (want[[3, 50, 192]] == 0).all()


@pytest.mark.parametrize("D,m", [(32, 8), (96, 8), (256, 4), (64, 64)])
def test_pq_encode_random_inputs_choose_a_nearest_codeword(D, m):
    """Random normal inputs.  With r the fp32 residual (part of the definition) a computed distance is the true one times (1 + t),
    |t| <= gamma_(dsub + 3): the difference is rounded once (its square carries 2 u), the product once, and the dsub non-negative
    terms are summed recursively.  The chosen codeword's computed distance is <= the true nearest one's, so in float64
    d_chosen - d_min <= gamma_(dsub + 3) * (d_chosen + d_min).  The kernel also promises the reference's own fp32 order of
    operations (no fused multiply-add), so the codes are the restatement's bit for bit."""
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(D + m)
    N, nlist, dsub = 777, 9, D // m
    x = rng.standard_normal((N, D)).astype(np.float32)
    cen = (0.3 * rng.standard_normal((nlist, D))).astype(np.float32)
    assign = rng.integers(0, nlist, size=N)
    cb = (0.8 * rng.standard_normal((m, R.KSUB, dsub))).astype(np.float32)
    got = ops.pq_encode(_dev(x), _dev(cb), _dev(assign), _dev(cen)).cpu().numpy().view(np.uint32)
    r, _ = R.residuals(x, assign, cen)
    d64 = R.distances(r, cb, dtype=np.float64)
    codes = R.code_bytes(got, m)
    chosen = np.take_along_axis(d64, codes[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    best = d64.min(axis=2)
    bound = R.gamma(dsub + 3) * (chosen + best)
    ratio = float(((chosen - best) / bound).max())
    print("pq_encode D %d m %d: max (d_chosen - d_min) / bound = %.3f" % (D, m, ratio))
    assert ((chosen - best) <= bound).all()
    np.testing.assert_array_equal(got, R.encode(x, cb, assign, cen))


# ---- packing -------------------------------------------------------------------------------------------------------------------------
def test_ivf_pack_moves_code_words_bit_for_bit():
    """ops.ivf_pack on the code words viewed as fp32 gives the word-plane-major list layout with the row numbers as identifiers, and
    every bit pattern survives the trip through a float register: all ones, quiet and signalling NaNs, denormals."""
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(3)
    sizes = np.array([0, 1, 63, 64, 65, 130])
    nlist, N, mw = len(sizes), int(sizes.sum()), 2
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes))
    words = rng.integers(0, 2 ** 32, size=(N, mw), dtype=np.uint64).astype(np.uint32)
    special = np.array([0xFFFFFFFF, 0x7FC00001, 0x7F800001, 0xFFC00000, 0xFF800001, 0x00000001, 0x807FFFFF, 0x7F800000, 0x80000000],
                       dtype=np.uint32)
    words[:len(special), 0] = special
    words[-len(special):, 1] = special[::-1]
    order, list_start = ops.ivf_build_lists(_dev(assign), nlist)
    np.testing.assert_array_equal(order.cpu().numpy(), np.argsort(assign, kind="stable"))
    packed, rows, blk_off = ops.ivf_pack(_words_dev(words).view(torch.float32), order, list_start, None)
    w_packed, w_rows, w_blk = R.pack(words, order.cpu().numpy(), list_start.cpu().numpy())
    np.testing.assert_array_equal(blk_off.cpu().numpy(), w_blk)
    assert w_blk.tolist() == [0, 0, 1, 2, 3, 5, 8]
    np.testing.assert_array_equal(rows.cpu().numpy(), w_rows)
    np.testing.assert_array_equal(packed.view(torch.int32).cpu().numpy().view(np.uint32), w_packed)


# ---- ivfpq_scan ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_index(m):
    """an integer-grid index: 6 lists of 0 .. 300 members (one empty, one with a single vector, three of more than one block)"""
    rng = np.random.default_rng(m)
    dsub = 2
    D = m * dsub
    sizes = np.array([150, 1, 300, 0, 70, 179])
    nlist, N = len(sizes), int(sizes.sum())
    assign = rng.permutation(np.repeat(np.arange(nlist), sizes))
    cen = rng.integers(-3, 4, size=(nlist, D)).astype(np.float32)
    cb = rng.integers(-4, 5, size=(m, R.KSUB, dsub)).astype(np.float32)
    codes = rng.integers(0, R.KSUB, size=(N, m)).astype(np.uint8)
    codes[:20] = 255                                                             # the highest code in every byte of a word
    order = np.argsort(assign, kind="stable")
    list_start = np.concatenate([[0], np.cumsum(sizes)])
    packed, rows, blk_off = R.pack(R.code_words(codes), order, list_start)
    q = rng.integers(-3, 4, size=(67, D)).astype(np.float32)
    dev = dict(packed=_words_dev(packed), rows=_dev(rows), blk_off=_dev(blk_off), cb=_dev(cb))
    return dict(D=D, nlist=nlist, assign=assign, cen=cen, cb=cb, codes=codes, q=q, dev=dev)


@pytest.mark.parametrize("m", [4, 8, 32, 64])
def test_ivfpq_scan_integer_grids_bit_for_bit(m):
    """small integers: the lookup tables, the coarse scores and every partial sum are exact in fp32, so scores and rows equal the
    float64 search exactly -- ties (plenty, on such a grid) to the lower row.  k in {1, 10, 128} x nprobe in {1, 3, nlist} x
    Bq in {1, 5, 67}; an empty list among the probed ones, a -1 probe, fewer than k members (the (-inf, -1) tail)."""
    from deep_recommenders_amd import ops
    c = _grid_index(m)
    nlist, dev = c["nlist"], c["dev"]
    rng = np.random.default_rng(100 + m)
    saw_tail = saw_tie = False
    for nprobe in (1, 3, nlist):
        for Bq in (1, 5, 67):
            q = c["q"][:Bq]
            probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(Bq)]).astype(np.int64)
            probes[0, 0] = 1 if nprobe == 1 else 3                              # the single-member list alone / the empty list first
            if nprobe == 3 and Bq > 1:
                probes[1, 1] = -1
            coarse = q.astype(np.float64) @ c["cen"].astype(np.float64).T
            ps = np.take_along_axis(coarse, np.clip(probes, 0, None), axis=1).astype(np.float32)
            for k in (1, 10, 128):
                s, i = ops.ivfpq_scan(_dev(q), _dev(probes), _dev(ps), dev["blk_off"], dev["packed"], dev["rows"], dev["cb"], k)
                want_s, want_i = R.adc_search(q, c["cen"], c["cb"], c["codes"], c["assign"], probes, k)
                what = "m %d nprobe %d Bq %d k %d" % (m, nprobe, Bq, k)
                np.testing.assert_array_equal(i.cpu().numpy(), want_i, err_msg=what)
                np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), want_s, err_msg=what)
                saw_tail |= bool((want_i == -1).any())
                saw_tie |= bool(((want_s[:, 1:] == want_s[:, :-1]) & (want_i[:, 1:] >= 0)).any())
    assert saw_tail and saw_tie


def _complete_adc_check(what, q, cen, cb, codes, assign, probes, s, i, k, probe_terms):
    """every returned score within its bound of the float64 ADC score of the returned row; the list sorted (score descending, ties to
    the lower row); every member of the probed lists returned when there are at most k, and otherwise no member left out whose
    float64 score exceeds the k-th returned one's by more than the two bounds"""
    m, _, dsub = cb.shape
    S = R.adc_scores(q, cen, cb, codes, assign)
    coarse_abs, lut_abs = R.adc_abs(q, cen, cb, codes, assign)
    B = R.adc_bound(coarse_abs, lut_abs, coarse_abs * (1.0 + 1e-6), m, dsub, probe_terms)
    worst, worst_out = 0.0, -np.inf
    for b in range(len(q)):
        mem = R.members(assign, probes[b])
        n = min(k, len(mem))
        rows, sc = i[b], s[b].astype(np.float64)
        assert (rows[n:] == -1).all() and np.isneginf(sc[n:]).all(), what
        rows, sc = rows[:n], sc[:n]
        assert len(set(rows.tolist())) == n and np.isin(rows, mem).all(), what
        err = np.abs(sc - S[b, rows])
        worst = max(worst, float((err / B[b, rows]).max()) if n else 0.0)
        assert (err <= B[b, rows]).all(), "%s: query %d, max |err| / bound = %.3f" % (what, b, float((err / B[b, rows]).max()))
        d = np.diff(sc)
        assert (d <= 0).all() and (np.diff(rows)[d == 0] > 0).all(), what
        if len(mem) > k:
            out = np.setdiff1d(mem, rows)
            kth = rows[-1]
            excess = S[b, out] - S[b, kth]
            allowed = B[b, out] + B[b, kth]
            worst_out = max(worst_out, float((excess / allowed).max()))
            assert (excess <= allowed).all(), "%s: query %d leaves out a better candidate: %.3f bounds" % (what, b, float((excess / allowed).max()))
    print("%s: max |score err| / bound = %.3f, max (left-out - k-th) / bounds = %.3f" % (what, worst, worst_out))


@functools.lru_cache(maxsize=None)
def _random_index(N, D, m, nlist):
    rng = np.random.default_rng(N + D)
    cand = rng.standard_normal((N, D)).astype(np.float32)
    cen = cand[rng.permutation(N)[:nlist]].copy() * 0.5
    assign = np.argmax(cand.astype(np.float64) @ cen.astype(np.float64).T, axis=1)
    r, _ = R.residuals(cand, assign, cen)
    pick = rng.permutation(N)[:R.KSUB]
    cb = np.ascontiguousarray(r[pick].reshape(R.KSUB, m, D // m).transpose(1, 0, 2))
    words = R.encode(cand, cb, assign, cen)
    return dict(cand=cand, cen=cen, assign=assign, cb=cb, words=words, codes=R.code_bytes(words, m))


@pytest.mark.parametrize("N,D,m,nlist,nprobe,Bq,k", [(5000, 32, 8, 16, 4, 64, 20), (4000, 96, 8, 16, 16, 64, 128)])
def test_ivfpq_scan_random_inputs_complete_check(N, D, m, nlist, nprobe, Bq, k):
    """Random normal inputs, the lists built and packed on the device.  The coarse scores handed to the scan are the float64 ones
    rounded to fp32 (one rounding: probe_terms = 1), so the bound is the scan's own arithmetic -- see ivfpq_ref.adc_bound."""
    from deep_recommenders_amd import ops
    c = _random_index(N, D, m, nlist)
    rng = np.random.default_rng(k)
    q = rng.standard_normal((Bq, D)).astype(np.float32)
    coarse = q.astype(np.float64) @ c["cen"].astype(np.float64).T
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :nprobe].astype(np.int64)
    ps = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
    order, list_start = ops.ivf_build_lists(_dev(c["assign"]), nlist)
    packed, rows, blk_off = ops.ivf_pack(_words_dev(c["words"]).view(torch.float32), order, list_start, None)
    s, i = ops.ivfpq_scan(_dev(q), _dev(probes), _dev(ps), blk_off, packed, rows, _dev(c["cb"]), k)
    s2, i2 = ops.ivfpq_scan(_dev(q[7:9]), _dev(probes[7:9]), _dev(ps[7:9]), blk_off, packed.view(torch.int32), rows, _dev(c["cb"]), k)
    assert torch.equal(s[7:9], s2) and torch.equal(i[7:9], i2)                  # a query's result does not depend on its batch
    _complete_adc_check("ivfpq_scan N %d D %d k %d" % (N, D, k), q, c["cen"], c["cb"], c["codes"], c["assign"], probes,
                        s.cpu().numpy(), i.cpu().numpy(), k, probe_terms=1)


# ---- rerank_topk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kin,k", [(20, 128, 128), (130, 5, 10), (64, 70, 10), (7, 64, 1)])
def test_rerank_topk_integer_grids_bit_for_bit(D, kin, k):
    """exact inner products on small integers == float64; duplicated candidate rows tie and the lower row comes first; -1 entries are
    none; kin < k leaves the (-inf, -1) tail"""
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(D + kin)
    N, Bq = 300, 9
    cand = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    cand[150:200] = cand[:50]                                                    # exact ties between rows r and r + 150
    q = rng.integers(-3, 4, size=(Bq, D)).astype(np.float32)
    rows = np.stack([rng.permutation(N)[:kin] for _ in range(Bq)]).astype(np.int64)
    rows[0, :min(kin, 4)] = [10, 160, 5, 155][:min(kin, 4)]
    rows[1, ::3] = -1
    rows[2] = -1                                                                 # nothing named
    s, i = ops.rerank_topk(_dev(q), _dev(cand), _dev(rows), k)
    want_s, want_i = R.rerank(q, cand, rows, k)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), want_s)
    assert (want_i[2] == -1).all() and (kin >= k or (want_i[:, kin:] == -1).all())


@pytest.mark.parametrize("D,kin,k", [(32, 128, 20), (200, 100, 100)])
def test_rerank_topk_random_inputs_within_the_derived_bound(D, kin, k):
    from deep_recommenders_amd import ops
    rng = np.random.default_rng(D)
    N, Bq = 1000, 33
    cand = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((Bq, D)).astype(np.float32)
    rows = np.stack([rng.permutation(N)[:kin] for _ in range(Bq)]).astype(np.int64)
    rows[3, 5:9] = -1
    s, i = ops.rerank_topk(_dev(q), _dev(cand), _dev(rows), k)
    s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
    S = q.astype(np.float64) @ cand.astype(np.float64).T
    B = R.rerank_bound(np.abs(q).astype(np.float64) @ np.abs(cand).astype(np.float64).T, D)
    worst, worst_out = 0.0, -np.inf
    for b in range(Bq):
        named = rows[b][rows[b] >= 0]
        n = min(k, len(named))
        assert (i[b, n:] == -1).all() and len(set(i[b, :n].tolist())) == n and np.isin(i[b, :n], named).all()
        r = i[b, :n]
        err = np.abs(s[b, :n] - S[b, r])
        worst = max(worst, float((err / B[b, r]).max()))
        assert (err <= B[b, r]).all()
        d = np.diff(s[b, :n])
        assert (d <= 0).all() and (np.diff(r)[d == 0] > 0).all()
        out = np.setdiff1d(named, r)
        if len(out):
            excess, allowed = S[b, out] - S[b, r[-1]], B[b, out] + B[b, r[-1]]
            worst_out = max(worst_out, float((excess / allowed).max()))
            assert (excess <= allowed).all()
    print("rerank_topk D %d: max |score err| / bound = %.3f, max (left-out - k-th) / bounds = %.3f" % (D, worst, worst_out))


# ---- FaissIVFPQ ----------------------------------------------------------------------------------------------------------------------
N_IDX, D_IDX, M_IDX = 5000, 32, 8


@functools.lru_cache(maxsize=None)
def _built():
    from deep_recommenders_amd.keras.models.retrieval import factorized_top_k as ftk
    rng = np.random.default_rng(42)
    cand = rng.standard_normal((N_IDX, D_IDX)).astype(np.float32)
    q = rng.standard_normal((64, D_IDX)).astype(np.float32)
    idx = ftk.FaissIVFPQ(k=20, nlist=16, nprobe=4, m=M_IDX).index(torch.tensor(cand))
    return idx, cand, q


def test_faiss_ivfpq_codes_are_the_restatement_of_its_own_state():
    """_codes == ref.encode(candidates, the index's centroids, assignments and codebooks).  A code whose two best float64 distances
    are closer than the encode bound (gamma_(dsub + 3) * their sum) may legitimately differ and is exempt; at most 1 % may be."""
    idx, cand, _ = _built()
    cen, cb = idx._centroids.cpu().numpy(), idx._codebooks.cpu().numpy()
    asg = idx._assignments.cpu().numpy()
    assert cen.shape == (16, D_IDX) and cb.shape == (M_IDX, R.KSUB, D_IDX // M_IDX) and np.isfinite(cb).all() and np.isfinite(cen).all()
    np.testing.assert_array_equal(asg, np.argmax(cand.astype(np.float64) @ cen.astype(np.float64).T, axis=1))
    got = R.code_bytes(idx._codes.cpu().numpy(), M_IDX)
    want = R.code_bytes(R.encode(cand, cb, asg, cen), M_IDX)
    r, _ = R.residuals(cand, asg, cen)
    two = np.sort(R.distances(r, cb, dtype=np.float64), axis=2)[:, :, :2]
    exempt = (two[:, :, 1] - two[:, :, 0]) <= R.gamma(D_IDX // M_IDX + 3) * (two[:, :, 1] + two[:, :, 0])
    print("FaissIVFPQ codes: %.4f %% exempt as near-ties, %d of %d differ" % (100.0 * exempt.mean(), int((got != want).sum()), got.size))
    assert exempt.mean() <= 0.01
    assert ((got == want) | exempt).all()
    for j in range(M_IDX):
        assert len(np.unique(got[:, j])) > 1                                    # every codebook has more than one codeword in use


def test_faiss_ivfpq_call_passes_the_complete_adc_check():
    """call() against the index's own state.  The coarse score reaches the scan from ops.topk_mips: an fp32 inner product of D terms
    whose operands the scan may have split into two fp16 terms each (22 of 24 significand bits: 4 u per operand), so
    probe_terms = D + 10 covers gamma_D, the two operands' representation error and the second-order terms."""
    from deep_recommenders_amd import ops
    idx, cand, q = _built()
    s, i = idx(torch.tensor(q))
    assert tuple(s.shape) == (64, 20) and i.dtype == torch.int64
    _, probes = ops.topk_mips(torch.tensor(q).cuda(), idx._centroids, 4)
    cb = idx._codebooks.cpu().numpy()
    _complete_adc_check("FaissIVFPQ.call", q, idx._centroids.cpu().numpy(), cb, R.code_bytes(idx._codes.cpu().numpy(), M_IDX),
                        idx._assignments.cpu().numpy(), probes.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), 20, probe_terms=D_IDX + 10)
    s5, i5 = idx(torch.tensor(q), k=5)                                          # the k override: a prefix of the same order
    assert torch.equal(s5, s[:, :5]) and torch.equal(i5, i[:, :5])
    s_again, i_again = idx(torch.tensor(q))
    assert torch.equal(s, s_again) and torch.equal(i, i_again)                  # bit-identical from run to run


def test_faiss_ivfpq_state_dict_round_trip_and_identifiers():
    from deep_recommenders_amd.keras.models.retrieval import factorized_top_k as ftk
    idx, cand, q = _built()
    s, i = idx(torch.tensor(q))
    state = idx.state_dict()
    assert sorted(state) == ["_blk_off", "_centroids", "_codebooks", "_packed_codes", "_packed_rows"]
    clone = ftk.FaissIVFPQ(k=20, nlist=16, nprobe=4, m=M_IDX)
    for name, value in state.items():
        setattr(clone, name, value.clone())
    s2, i2 = clone(torch.tensor(q))
    assert torch.equal(s, s2) and torch.equal(i, i2)
    rng = np.random.default_rng(7)
    ids = rng.permutation(10 * N_IDX)[:N_IDX].astype(np.int64) + 2 ** 33
    for identifiers in (torch.tensor(ids), torch.tensor(ids % 1000, dtype=torch.float32) + 0.5):
        withid = ftk.FaissIVFPQ(k=8, nlist=16, nprobe=1, m=M_IDX, refine=2).index(torch.tensor(cand[:600]), identifiers[:600])
        s_id, got = withid(torch.tensor(q))
        assert "_ids" in withid.state_dict() and "_vectors" in withid.state_dict()
        kept, withid._ids = withid._ids, None
        s_row, rows = withid(torch.tensor(q))                                   # the same search, row numbers out
        assert torch.equal(s_id, s_row) and got.dtype == identifiers.dtype
        rows = rows.cpu().numpy()
        want = np.where(rows >= 0, identifiers.numpy()[np.clip(rows, 0, None)], -1 if identifiers.dtype == torch.int64 else np.nan)
        if identifiers.dtype == torch.int64:
            np.testing.assert_array_equal(got.cpu().numpy(), want)
        else:
            found = rows >= 0
            np.testing.assert_array_equal(got.cpu().numpy()[found], want[found])
        assert (rows >= 0).any()
        withid._ids = kept


def test_faiss_ivfpq_refine_is_exact_over_the_probed_list():
    """N 400, nlist 16, nprobe 1, normalize=True, k 10, refine 13: the scan returns min(130, 128) = 128 rows, so with no list above
    128 members every member of the probed list is re-scored exactly and the answer is the exact search over that list -- on unit
    vectors on both sides (normalize=True), rows exactly, scores to 1e-5."""
    from deep_recommenders_amd import ops
    from deep_recommenders_amd.keras.models.retrieval import factorized_top_k as ftk
    rng = np.random.default_rng(11)
    cand = (rng.standard_normal((400, D_IDX)) * rng.uniform(0.5, 3.0, size=(400, 1))).astype(np.float32)
    q = (rng.standard_normal((48, D_IDX)) * rng.uniform(0.5, 3.0, size=(48, 1))).astype(np.float32)
    idx = ftk.FaissIVFPQ(k=10, nlist=16, nprobe=1, m=M_IDX, normalize=True, refine=13).index(torch.tensor(cand))
    asg = idx._assignments.cpu().numpy()
    largest = int(np.bincount(asg, minlength=16).max())
    assert largest <= 128, "precondition: the largest list has %d members" % largest
    s, i = idx(torch.tensor(q))
    cn = cand.astype(np.float64) / np.linalg.norm(cand.astype(np.float64), axis=1, keepdims=True)
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    np.testing.assert_allclose(idx._vectors.cpu().numpy(), cn, rtol=0, atol=1e-6)
    _, probes = ops.topk_mips(ftk._normalize_L2(torch.tensor(q).cuda()), idx._centroids, 1)
    want_s, want_i = R.ivf_exact_search(qn, cn, asg, probes.cpu().numpy(), 10)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    found = want_i >= 0
    np.testing.assert_allclose(s.cpu().numpy()[found], want_s[found], rtol=0, atol=1e-5)
    assert np.isneginf(s.cpu().numpy()[~found]).all() and float(s.max()) <= 1.0 + 1e-5
    print("refine: largest list %d, %d of %d slots found" % (largest, int(found.sum()), found.size))


# ---- EBR -----------------------------------------------------------------------------------------------------------------------------
def _toy_model_and_inputs(n_docs, n_queries, seed):
    """an untrained EBR over two small identity columns per side, and token-bag inputs drawn per topic"""
    from deep_recommenders_amd import feature_column as fc
    from deep_recommenders_amd.keras.models.retrieval import EBR

    def columns(prefix):
        return [fc.embedding_column(fc.categorical_column_with_identity(prefix + "_tokens", 96), 8),
                fc.embedding_column(fc.categorical_column_with_identity(prefix + "_place", 6), 8)]
    model = EBR(columns("query"), columns("doc"), [32, 16], seed=seed).build()
    rng = np.random.default_rng(seed)

    def inputs(prefix, B):
        topic = rng.integers(0, 8, size=B)
        bag = topic[:, None] * 12 + rng.integers(0, 12, size=(B, 5))
        return {prefix + "_tokens": torch.from_numpy(bag).cuda(), prefix + "_place": torch.from_numpy(rng.integers(0, 6, size=(B, 1))).cuda()}
    return model, inputs("doc", n_docs), inputs("query", n_queries)


def test_ebr_serves_through_the_ivfpq_index():
    """EBR.index(kind="ivfpq") with every list probed and refine: the brute-force answer -- the same identifiers wherever the
    brute-force score gap on both sides exceeds 1e-5, and the scores to 1e-5"""
    model, docs, queries = _toy_model_and_inputs(300, 32, 3)
    idents = torch.arange(300, dtype=torch.int64) * 5 + 3
    model.index(docs, identifiers=idents.cuda(), k=11, kind="brute_force")
    s_a, i_a = model.top_k(queries, 11)
    served = model.index(docs, identifiers=idents.cuda(), k=10, kind="ivfpq", nlist=4, nprobe=4, m=4, refine=13)
    from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import FaissIVFPQ
    assert isinstance(served, FaissIVFPQ)
    s_b, i_b = model.top_k(queries, 10)
    s_a, i_a, s_b, i_b = s_a.cpu().numpy().astype(np.float64), i_a.cpu().numpy(), s_b.cpu().numpy().astype(np.float64), i_b.cpu().numpy()
    np.testing.assert_allclose(s_b, s_a[:, :10], rtol=0, atol=1e-5)
    gap = -np.diff(s_a, axis=1)                                                  # gap[:, t] = s[t] - s[t + 1]
    clear = gap[:, :10] > 1e-5
    clear[:, 1:] &= gap[:, :9] > 1e-5
    print("EBR ivfpq: %d of %d positions have a clear brute-force gap" % (int(clear.sum()), clear.size))
    assert clear.any() and (i_b[clear] == i_a[:, :10][clear]).all()
    assert set(i_b.reshape(-1).tolist()) <= set(idents.tolist())
