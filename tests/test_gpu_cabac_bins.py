"""GPU: the bin collector and walk of the CABAC size pricing's header part (csrc/cabac_rd.hip.h cab_put / cab_walk_a: every context's bins of a macroblock
as one bit string in the lane that owns the context, walked through the chain table eight bins a lookup) through the primitive x264gpu_cabac_bins_walk, against
the bin-by-bin restatement tests/cabac_bins_ref.py: same context variables, same bits, in every case."""
import numpy as np
import pytest

import cabac_bins_ref as R

pytestmark = pytest.mark.gpu

N = 1500


def test_cabac_bins_walk_primitive_vs_serial_restatement(gpu):
    import torch
    lib = gpu
    cases = R.cases(N, 0xb175)
    assert len(cases) == N
    # ---- the cases hold what they are there for ----
    counts = [R.bins_on(t) for t, _ in cases]
    per_ctx = [set(c.values()) for c in counts]
    for k in R.EXACT:
        assert any(k in s for s in per_ctx), f"no context with exactly {k} bins"
    assert any(max(c.values(), default=0) > 64 for c in counts) and any(max(c.values(), default=0) > 128 for c in counts)
    assert any(not t for t, _ in cases)                                                             # the empty list
    assert any(any(c < 64 for c in cn) and any(c >= 64 for c in cn) for cn in counts)               # both registers in one case
    assert any(63 in cn and 64 in cn for cn in counts) and any(104 in cn and 399 in cn for cn in counts)      # neighbours across the register split
    twins = [i for i in range(1, N) if cases[i][0] != cases[i - 1][0] and cases[i][0] == R.one_by_one(cases[i - 1][0]) and cases[i][1] == cases[i - 1][1]]
    assert len(twins) > 100                                                                         # runs in one go | the same bins one by one
    seen = set().union(*[set(c) for c in counts])
    assert seen == set(R.CONTEXTS)
    # ---- device ----
    first = np.zeros(N + 1, np.int32)
    first[1:] = np.cumsum([len(t) for t, _ in cases])
    tri = np.array([x for t, _ in cases for x in t], np.int32).reshape(-1, 3)
    st_in = np.array([s for _, s in cases], np.uint8)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_t, d_f, d_s = d(tri), d(first), d(st_in)
    d_so, d_b = torch.zeros_like(d_s), torch.zeros(N, dtype=torch.int32, device="cuda")
    lib.check(lib.x264gpu_cabac_bins_walk(d_t.data_ptr(), d_f.data_ptr(), N, d_s.data_ptr(), d_so.data_ptr(), d_b.data_ptr(), None), "cabac_bins_walk")
    torch.cuda.synchronize()
    got_s, got_b = d_so.cpu().numpy(), d_b.cpu().numpy()
    # ---- the restatement ----
    want = [R.code(t, s) for t, s in cases]
    want_s, want_b = np.array([w[0] for w in want], np.uint8), np.array([w[1] for w in want], np.int32)
    bad = np.nonzero(got_b != want_b)[0]
    assert len(bad) == 0, f"bits differ in {len(bad)} of {N} cases; first {bad[0]}: {cases[bad[0]][0][:12]} device {got_b[bad[0]]} serial {want_b[bad[0]]}"
    bads = np.nonzero((got_s != want_s).any(axis=1))[0]
    assert len(bads) == 0, f"context variables differ in {len(bads)} of {N} cases; first {bads[0]}: contexts {np.nonzero(got_s[bads[0]] != want_s[bads[0]])[0].tolist()}"
    for i in twins:
        assert got_b[i] == got_b[i - 1] and np.array_equal(got_s[i], got_s[i - 1])
    assert want_b.max() > 50000
