"""Serial restatement of the macroblock layer's own CABAC bins (mb_type .. mb_qp_delta, coded_block_flags: contexts 0..104 and 399..401) as the size pricing
counts them: one bin after the other through cabac_levels_ref.step — the checker of the device's per-context bin strings (csrc/cabac_rd.hip.h cab_put /
cab_walk_a, primitive x264gpu_cabac_bins_walk).  Test infrastructure: pure Python."""
import random

from cabac_levels_ref import step

CONTEXTS = list(range(105)) + [399, 400, 401]
EXACT = (8, 9, 32, 33, 48, 64)          # bins on one context: the eight-bin lookup's boundary, the string widths' boundaries (32 / 64 bits)
MORE = (65, 100, 128, 129, 200)         # ... and beyond: a second walk, a third


def code(triples, states):
    """(context, bin, repeat) triples in coding order on the 460 context variables -> the variables afterwards, the bits in 1/256"""
    st, bits = list(states), 0
    for ctx, b, rep in triples:
        for _ in range(rep):
            st[ctx], co = step(st[ctx], b)
            bits += co
    return st, bits


def bins_on(triples):
    """bins per context of a case"""
    n = {}
    for ctx, _, rep in triples:
        n[ctx] = n.get(ctx, 0) + rep
    return n


def one_by_one(triples):
    return [(ctx, b, 1) for ctx, b, rep in triples for _ in range(rep)]


def _single(rnd, ctx, n):
    """n bins on one context, each its own triple"""
    p = rnd.random()
    return [(ctx, 1 if rnd.random() < p else 0, 1) for _ in range(n)]


def _random(rnd):
    kind = rnd.randrange(4)
    pool = CONTEXTS if kind else rnd.sample(CONTEXTS, rnd.randint(1, 4))          # (a few contexts only: long strings)
    p = rnd.random()
    out = []
    for _ in range(rnd.choice([1, 3, 8, 20, 40, 70])):
        rep = rnd.choice([1, 1, 1, 1, 2, 3, 4, 5, 8, 9, 13, 30, 51]) if kind != 3 else 1
        out.append((rnd.choice(pool), 1 if rnd.random() < p else 0, rep))
    return out


def cases(n, seed):
    """n cases: (triples, the 460 context variables before).  The first ones are the boundaries the device's form has; then every run-length case is
    followed by the same bins one by one; the rest is random"""
    rnd = random.Random(seed)
    lists = [[]]
    for k in EXACT + MORE:
        lists.append(_single(rnd, rnd.randrange(64), k))                       # register a0
        lists.append(_single(rnd, rnd.choice(CONTEXTS[64:]), k))               # register a1
        lists.append([(rnd.choice(CONTEXTS), rnd.randrange(2), k)])            # as one run
    lists.append(_single(rnd, 10, 5) + _single(rnd, 70, 5))
    for pair in ((63, 64), (104, 399)):
        t = _single(rnd, pair[0], 12) + _single(rnd, pair[1], 12)
        rnd.shuffle(t)
        lists.append(t)
    while len(lists) < n:
        t = _random(rnd)
        lists.append(t)
        if any(rep > 1 for _, _, rep in t) and len(lists) < n:
            lists.append(one_by_one(t))
    out = [(t, [rnd.randrange(126) for _ in range(460)]) for t in lists]
    # a run and its one-by-one twin start from the same variables
    for i in range(1, len(out)):
        if out[i][0] and out[i][0] == one_by_one(out[i - 1][0]) and out[i][0] != out[i - 1][0]:
            out[i] = (out[i][0], list(out[i - 1][1]))
    return out
