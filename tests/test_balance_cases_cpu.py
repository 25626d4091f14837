"""CPU: the cases of tests/balance_cases.py reach what they claim, on the checker alone — tests/test_gpu_balance.py then holds the device's permuted lock-step
batch against these very sessions.  A batch can only show a wrong per-stream index where the streams' right answers differ, and the balancer only moves
streams whose times differ: so the sequences must code differently picture by picture, their work must be spread widely, and the per-stream controls
(quantisers, direct modes) must change what is coded.  These are conditions on the inputs: a sequence that fails one is to be replaced."""
import itertools

import numpy as np
import pytest

import balance_cases as BC
import oracle_lib as O


@pytest.mark.parametrize("S", BC.PERM_COUNTS)
def test_perm_ref_is_a_permutation(S):
    for name, t in BC.wtime_arrays(S).items():
        assert t.dtype == np.uint32 and t.shape == (S,)
        p = BC.perm_ref(t)
        assert np.array_equal(np.sort(p), np.arange(S)), name


def test_perm_ref_by_hand():
    # ranks: stream 2 (9), 0 (7), 3 (7), 4 (5), 1 (1); half = 3: the slower three in order, the faster two backwards
    assert BC.perm_ref([7, 1, 9, 7, 5]).tolist() == [2, 0, 3, 1, 4]
    assert BC.perm_ref([4, 4, 4, 4]).tolist() == [0, 1, 3, 2]
    assert BC.perm_ref([3]).tolist() == [0]
    assert BC.perm_ref([0, 0xffffffff]).tolist() == [1, 0]
    # the slowest stream takes workgroup 0, the fastest the one behind the slower half (workgroups n and n + 1024 share a SIMD: half = 1024 at 2048 streams)
    t = BC.wtime_arrays(2048)["random32"]
    p = BC.perm_ref(t)
    assert p[0] == np.argmax(t) and p[1024] == np.argmin(t)


@pytest.mark.parametrize("S", [BC.S_DEFAULT, BC.S_BIG])
def test_the_deal_of_sequences(S):
    seq = [BC.seq_of(s, S) for s in range(S)]
    assert seq[0] == BC.FLAT[0] and seq[-1] == BC.FLAT[1] and set(seq) == set(range(BC.K))
    for s in range(S):
        for d in (1, 16):
            assert s + d >= S or seq[s] != seq[s + d], (s, d)
    off, mv = BC.side_rows(S)
    assert off.shape == (S, BC.NMB) and off.dtype == np.float32 and np.abs(off).max() <= 6 and mv.shape == (S, BC.NMB, 2)


def _sessions(case):
    if case == "ip":
        return [BC.ip_session(k) for k in range(BC.K)]
    if case == "b":
        return [BC.b_session(k, 0, 0, 0) for k in range(BC.K)]
    if case == "nr":
        return [BC.nr_plain_session(k) for k in range(BC.K)]
    S = BC.S_DEFAULT          # side rows: the first stream of every sequence, with its own offsets and vectors
    first = {}
    for s in range(S):
        first.setdefault(BC.seq_of(s, S), s)
    return [BC.side_session(first[k], S) for k in range(BC.K)]


@pytest.mark.parametrize("case", ["ip", "b", "side", "nr"])
def test_sequences_code_differently_in_every_picture(case):
    ses = _sessions(case)
    for i in range(len(ses[0])):
        recons = [s[i]["recon"].tobytes() for s in ses]
        assert len(set(recons)) == BC.K, f"{case} picture {i}: two sequences reconstruct alike"
        coded = [k for k in range(BC.K) if ses[k][i]["lv"].any()]
        assert set(range(BC.K)) - set(coded) <= set(BC.FLAT), f"{case} picture {i}: {[BC.seq_name(k) for k in range(BC.K) if k not in coded]} code nothing"
        assert len({ses[k][i]["lv"].tobytes() for k in coded}) == len(coded) >= BC.K - 2, f"{case} picture {i}: two sequences' levels are alike"
        for a, b in itertools.combinations(range(BC.K), 2):
            assert a in BC.FLAT and b in BC.FLAT or ses[a][i]["mb"].tobytes() != ses[b][i]["mb"].tobytes(), f"{case} picture {i}: records of {a} and {b} alike"


def test_the_work_is_spread():
    """in every P and B picture of the headline case the flat sequences skip (nearly) everything and full-range noise skips nothing"""
    cheap = (O.MB_P_SKIP, O.MB_B_SKIP, O.MB_B_DIRECT)
    for k in BC.FLAT + (BC.NOISE_FULL,):
        for q in range(3):
            for i, p in enumerate(BC.b_session(k, q, 0, 0)):
                if p["pt"] <= 1:
                    continue
                n = int(np.isin(p["mb"]["type"], cheap).sum())
                print(f"{BC.seq_name(k)} qp +{q} picture {i} (type {p['pt']}): {n} of {BC.NMB} skipped or direct")
                assert n == 0 if k == BC.NOISE_FULL else n >= 10, (BC.seq_name(k), q, i, n)


def test_per_stream_controls_change_the_outcome():
    lv = lambda ses: b"".join(p["lv"].tobytes() for p in ses)
    for k in range(BC.K):
        if k in BC.FLAT:
            continue
        assert len({lv(BC.b_session(k, q, 0, 0)) for q in range(3)}) == 3, f"{BC.seq_name(k)}: two quantisers code alike"
    # the float quantiser enters the AQ quantisers before the rounding: on some sequence it moves a macroblock's quantiser
    assert any(lv(BC.b_session(k, 0, q5, 0)) != lv(BC.b_session(k, 0, 0, 0)) for k in range(BC.K) for q5 in range(1, 5)), "the float quantiser moves nothing"
    moved = [k for k in range(BC.K)
             if any(a["mb"].tobytes() != b["mb"].tobytes() for a, b in zip(BC.b_session(k, 0, 0, 0), BC.b_session(k, 0, 0, 1)) if a["pt"] >= 3)]
    print("temporal direct changes records of", [BC.seq_name(k) for k in moved])
    assert moved, "spatial and temporal direct code alike everywhere"
    # --direct auto's probe counts differ between streams too (what direct_scores(s) is compared with)
    assert len({p["dscore"] for k in range(BC.K) for p in BC.b_session(k, 0, 0, 0) if p["pt"] >= 3}) > 4


def test_side_rows_change_the_outcome():
    """the same sequence under two streams' offsets and vectors codes differently (the rows are not decoration)"""
    S = BC.S_DEFAULT
    by_seq = {}
    for s in range(1, 200):
        by_seq.setdefault(BC.seq_of(s, S), []).append(s)
    k, (a, b) = next((k, v[:2]) for k, v in by_seq.items() if k not in BC.FLAT and len(v) >= 2)
    assert any(x["mb"].tobytes() != y["mb"].tobytes() for x, y in zip(BC.side_session(a, S), BC.side_session(b, S)))
    qp = BC.side_session(a, S)[1]["mb"]["qp"]
    assert len(np.unique(qp)) > 4, "the offsets reach the macroblocks' quantisers"
