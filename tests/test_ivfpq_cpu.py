"""CPU checks of the IVF-PQ index: the NumPy restatement (tests/ivfpq_ref.py) against the exact IVF search where quantisation loses
nothing, its own packing and tie rules, the argument errors of ops.pq_check / pq_encode / ivfpq_scan / rerank_topk (raised on CPU
tensors, before any device call) and FaissIVFPQ's error messages."""
import numpy as np
import pytest
import torch

import ivfpq_ref as R
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.retrieval import factorized_top_k as ftk


def test_adc_equals_the_exact_ivf_search_when_every_residual_sub_vector_is_a_codeword():
    """<= 256 distinct residual sub-vectors per subspace, all of them in the codebook: encode finds them at distance 0, the decoded
    residual is the residual, and q . c + sum_j LUT[j][code_j] == q . x.  Integer grids: every number is exact in fp32 and float64."""
    rng = np.random.default_rng(0)
    N, D, m, nlist, Bq, k = 600, 12, 4, 5, 9, 17
    dsub = D // m
    codebooks = rng.integers(-4, 5, size=(m, R.KSUB, dsub)).astype(np.float32)
    centroids = rng.integers(-3, 4, size=(nlist, D)).astype(np.float32)
    assign = rng.integers(0, nlist - 1, size=N)                                  # the last list stays empty
    pick = rng.integers(0, R.KSUB, size=(N, m))
    res = np.concatenate([codebooks[j, pick[:, j]] for j in range(m)], axis=1)
    cand = centroids[assign] + res
    q = rng.integers(-3, 4, size=(Bq, D)).astype(np.float32)
    words = R.encode(cand, codebooks, assign, centroids)
    codes = R.code_bytes(words, m)
    dec = np.concatenate([codebooks[j, codes[:, j]] for j in range(m)], axis=1)
    np.testing.assert_array_equal(dec, res)                                      # (a duplicated codeword may move the code, never the value)
    # ties go to the LOWER code: no earlier codeword of the codebook equals the chosen one's sub-vector
    for j in range(m):
        first = np.array([np.flatnonzero((codebooks[j] == codebooks[j, c]).all(axis=1))[0] for c in range(R.KSUB)])
        np.testing.assert_array_equal(codes[:, j], first[pick[:, j]])
    np.testing.assert_array_equal(R.code_words(codes), words)
    probes = np.stack([rng.permutation(nlist)[:3] for _ in range(Bq)])
    probes[2, 1] = -1                                                            # a skipped probe
    probes[3] = [nlist - 1, -1, -1]                                              # only the empty list: nothing found
    s_adc, i_adc = R.adc_search(q, centroids, codebooks, codes, assign, probes, k)
    s_ex, i_ex = R.ivf_exact_search(q, cand, assign, probes, k)
    np.testing.assert_array_equal(s_adc, s_ex)
    np.testing.assert_array_equal(i_adc, i_ex)
    assert (i_adc[3] == -1).all() and np.isneginf(s_adc[3]).all()
    # re-ranking the ADC rows with the vectors is the same answer here
    s_rr, i_rr = R.rerank(q, cand, i_adc, k)
    np.testing.assert_array_equal(s_rr, s_ex)
    np.testing.assert_array_equal(i_rr, i_ex)
    # a vector whose assignment is out of range encodes as zeros
    bad = assign.copy()
    bad[:3] = [-1, nlist, 10 ** 12]
    assert (R.encode(cand, codebooks, bad, centroids)[:3] == 0).all()


def test_reference_packing_is_word_plane_major_in_blocks_of_64():
    rng = np.random.default_rng(1)
    sizes = np.array([0, 1, 65, 64])
    N, mw = int(sizes.sum()), 2
    assign = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    order = np.argsort(assign, kind="stable")
    list_start = np.concatenate([[0], np.cumsum(sizes)])
    words = rng.integers(0, 2 ** 32, size=(N, mw), dtype=np.uint64).astype(np.uint32)
    packed, rows, blk_off = R.pack(words, order, list_start)
    assert blk_off.tolist() == [0, 0, 1, 3, 4] and packed.size == 4 * mw * 64 and rows.size == 4 * 64
    assert (rows >= 0).sum() == N and sorted(rows[rows >= 0].tolist()) == list(range(N))
    for slot in np.flatnonzero(rows >= 0):
        blk, lane = divmod(int(slot), 64)
        for w in range(mw):
            assert packed[(blk * mw + w) * 64 + lane] == words[rows[slot], w]
    members = rows[64:64 * 3][rows[64:64 * 3] >= 0]                              # list 2: input order kept
    assert members.tolist() == sorted(members.tolist()) and (assign[members] == 2).all()


def test_domain_errors_name_the_argument_and_come_before_any_device_call():
    assert ops.pq_check(64, 16) == (64, 16, 4) and ops.pq_check(1024, 64) == (1024, 64, 16) and ops.pq_check(256, 4) == (256, 4, 64)
    for D, m, word in [(64, 6, "m"), (64, 0, "m"), (128, 68, "m"), (66, 8, "multiple of m"), (1032, 24, "D"),
                       (520, 8, "D / m")]:
        with pytest.raises(ValueError, match=word):
            ops.pq_check(D, m)
    cb = torch.zeros(8, 256, 4)
    x = torch.zeros(10, 32)
    with pytest.raises(ValueError, match="codebooks"):
        ops.pq_encode(x, torch.zeros(8, 255, 4))
    with pytest.raises(ValueError, match="codebooks"):
        ops.pq_encode(x, torch.zeros(8, 256, 5))
    with pytest.raises(ValueError, match="multiple of m"):
        ops.pq_encode(torch.zeros(10, 36), cb)
    with pytest.raises(ValueError, match="pq_encode: x"):
        ops.pq_encode(x.double(), cb)
    with pytest.raises(ValueError, match="come together"):
        ops.pq_encode(x, cb, assign=torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="centroids"):
        ops.pq_encode(x, cb, assign=torch.zeros(10, dtype=torch.int64), centroids=torch.zeros(3, 31))
    with pytest.raises(ValueError, match="assign"):
        ops.pq_encode(x, cb, assign=torch.zeros(9, dtype=torch.int64), centroids=torch.zeros(3, 32))
    q = torch.zeros(5, 32)
    probes = torch.zeros(5, 2, dtype=torch.int64)
    ps = torch.zeros(5, 2)
    blk_off = torch.zeros(4, dtype=torch.int64)
    codes = torch.zeros(2 * 64 * 2, dtype=torch.int32)
    rows = torch.zeros(2 * 64, dtype=torch.int64)
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must lie"):
            ops.ivfpq_scan(q, probes, ps, blk_off, codes, rows, cb, k)
    with pytest.raises(ValueError, match="m must be"):
        ops.ivfpq_scan(q, probes, ps, blk_off, codes, rows, torch.zeros(2, 256, 16), 5)
    with pytest.raises(ValueError, match="probes"):
        ops.ivfpq_scan(q, probes[:, :0], ps[:, :0], blk_off, codes, rows, cb, 5)
    with pytest.raises(ValueError, match="probe_scores"):
        ops.ivfpq_scan(q, probes, ps[:, :1], blk_off, codes, rows, cb, 5)
    with pytest.raises(ValueError, match="packed_codes"):
        ops.ivfpq_scan(q, probes, ps, blk_off, codes[:-1], rows, cb, 5)
    with pytest.raises(ValueError, match="packed_rows"):
        ops.ivfpq_scan(q, probes, ps, blk_off, codes, rows[:-1], cb, 5)
    cand = torch.zeros(20, 32)
    with pytest.raises(ValueError, match="kin"):
        ops.rerank_topk(q, cand, torch.zeros(5, 129, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="k must lie"):
        ops.rerank_topk(q, cand, torch.zeros(5, 8, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="share D"):
        ops.rerank_topk(q, torch.zeros(20, 31), torch.zeros(5, 8, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="rows"):
        ops.rerank_topk(q, cand, torch.zeros(4, 8, dtype=torch.int64), 5)


def test_faiss_ivfpq_raises_the_messages_of_faiss():
    with pytest.raises(ValueError, match="must be called first"):
        ftk.FaissIVFPQ()(torch.zeros(3, 32))
    with pytest.raises(ValueError, match="ndim should be 2"):
        ftk.FaissIVFPQ().index(torch.zeros(5))
    with pytest.raises(ValueError, match=r"Number of training points \(255\) should be at least as large as number of clusters \(256\)"):
        ftk.FaissIVFPQ(m=8).index(torch.zeros(255, 32))
    with pytest.raises(ValueError, match=r"Number of training points \(300\) should be at least as large as number of clusters \(512\)"):
        ftk.FaissIVFPQ(m=8, nlist=512).index(torch.zeros(300, 32))
    with pytest.raises(ValueError, match="multiple of m"):
        ftk.FaissIVFPQ(m=8).index(torch.zeros(300, 36))
    with pytest.raises(ValueError, match="refine"):
        ftk.FaissIVFPQ(refine=-1)
    idx = ftk.FaissIVFPQ()
    idx._packed_codes = torch.zeros(64 * 2, dtype=torch.int32)                   # "indexed": the queries' type is checked next
    with pytest.raises(ValueError, match="Queries must be a tensor"):
        idx({"a": torch.zeros(3, 32)})
    with pytest.raises(ValueError, match="Queries must be a tensor"):
        idx([[0.0] * 32])
    assert issubclass(ftk.FaissIVFPQ, ftk.TopK)
    assert [n for n, _ in ftk.FaissIVFPQ().named_buffers()] == [] and "_codebooks" in ftk.FaissIVFPQ()._buffers
