"""CPU: the Python twin of the QP-RD walk (tests/qprd_ref.py) on hand-worked cases.  Every case names the costs of exactly the quantisers the walk may ask for: a
quantiser outside the worked list is a KeyError, so the order asked is pinned together with the choice."""
import pytest

import qprd_ref as R


def run(curve, orig, last, psy=0, t8=False, lo=1, hi=51, flip_cost=None):
    """curve: {q: cost} or {q: (cost, empty)}; flip_cost: {q: cost with the other transform size}"""
    def cost(q, flip):
        if flip:
            return flip_cost[q], False
        v = curve[q]
        return v if isinstance(v, tuple) else (v, False)
    qp, flip, asked = R.walk(cost, orig, last, lo, hi, psy, t8)
    assert all(f is False for _, f in asked[:-1])
    return qp, flip, [q for q, f in asked if not f], [q for q, f in asked if f]


def test_monotone_curve_walks_down_to_the_minimum():
    # up: 27 costs more, one failure > threshold 0.  down: 25, 24 improve, 23 fails.  last_qp == orig_qp was never walked over: asked for at the end
    assert run({26: 100, 27: 110, 25: 90, 24: 80, 23: 85}, 26, 26) == (24, False, [26, 27, 25, 24, 23, 26], [])


def test_a_tie_is_a_failure():
    assert run({26: 100, 27: 100, 25: 100}, 26, 26) == (26, False, [26, 27, 25, 26], [])
    # psy-rd on: one failure is tolerated.  up: 27 ties (1), 28 improves (0), 29 ties (1), 30 fails (2 > 1).  down: 25 ties (1), 24 fails (2)
    assert run({26: 100, 27: 100, 28: 99, 29: 99, 30: 120, 25: 100, 24: 101}, 26, 26, psy=1) == (28, False, [26, 27, 28, 29, 30, 25, 24, 26], [])


def test_threshold_by_direction_towards_last_qp():
    # last_qp below: the walk down tolerates one failure, the walk up none; 24 == last_qp is walked over, so it is not asked for again
    assert run({26: 100, 27: 105, 25: 101, 24: 95, 23: 96, 22: 97}, 26, 24) == (24, False, [26, 27, 25, 24, 23, 22], [])
    # last_qp above: mirrored
    assert run({26: 100, 27: 101, 28: 95, 29: 96, 30: 97, 25: 100}, 26, 28) == (28, False, [26, 27, 28, 29, 30, 25], [])
    # psy and towards last_qp: threshold 2 down (25: 1, 24: 2, 23 improves: 0, 22: 1, 21: 2, 20: 3 > 2), 1 up (27: 1, 28: 2 > 1)
    curve = {26: 100, 27: 105, 28: 106, 25: 101, 24: 102, 23: 90, 22: 91, 21: 92, 20: 93}
    assert run(curve, 26, 24, psy=1) == (23, False, [26, 27, 28, 25, 24, 23, 22, 21, 20], [])


def test_walk_up_ends_at_an_empty_cbp():
    # 27 improves and codes nothing: no point in going further up
    assert run({26: 100, 27: (90, True), 25: 100}, 26, 26) == (27, False, [26, 27, 25, 26], [])


def test_empty_cbp_at_orig_jump_down_breaks():
    # nothing coded at 26: only the walk down, begun with a jump to 26 - 0 - 1.  Still nothing coded there: over.  Its cost is NOT compared (50 < 100),
    # and last_qp = 26 > 25 counts as tried
    assert run({26: (100, True), 25: (50, True)}, 26, 26) == (26, False, [26, 25], [])
    # last_qp 24 below: threshold 1, jump to 26 - 1 - 1.  last_qp == the jump's quantiser is not above it: asked for at the end, and there its cost counts
    assert run({26: (100, True), 24: (50, True)}, 26, 24) == (24, False, [26, 24, 24], [])
    # last_qp 25 is above the jump's 24: it counts as tried, nothing more is asked
    assert run({26: (100, True), 24: (50, True)}, 26, 25) == (26, False, [26, 24], [])


def test_empty_cbp_at_orig_jump_down_succeeds_and_checked_qp_is_not_taken_as_best():
    # psy, last_qp 22 below: threshold 2, jump to 23, which codes something (cost 70: kept as checked_cost).  Walk: 25 (90: best), 24 (95: 1), 23 reused (70 < 95:
    # 0, but not compared with the best), 22 (80: best although 23 cost less; == last_qp; 80 >= 70: 1), 21 (2), 20 (3 > 2)
    curve = {26: (100, True), 23: 70, 25: 90, 24: 95, 22: 80, 21: 85, 20: 86}
    assert run(curve, 26, 22, psy=1) == (22, False, [26, 23, 25, 24, 22, 21, 20], [])


def test_last_qp_tried_last_and_winning():
    # out of the walk's reach (up, with one failure tolerated towards it, ends at 28, down at 25): asked for at the end, strictly cheaper, taken
    assert run({26: 100, 27: 101, 28: 102, 25: 101, 31: 99}, 26, 31) == (31, False, [26, 27, 28, 25, 31], [])
    # ... and a tie there changes nothing
    assert run({26: 100, 27: 101, 28: 102, 25: 101, 31: 100}, 26, 31) == (26, False, [26, 27, 28, 25, 31], [])


def test_walls():
    # the range ends both walks while they still improve
    assert run({26: 100, 27: 90, 25: 95}, 26, 26, lo=25, hi=27) == (27, False, [26, 27, 25, 26], [])
    # the jump down is clipped to qp_min (26 - 1 - 1 = 24 -> 25); the walk then reuses it and meets the wall
    assert run({26: (100, True), 25: 80}, 26, 26, psy=1, lo=25, hi=27) == (26, False, [26, 25, 26], [])


def test_qp_min_equals_qp_max():
    assert run({26: 100}, 26, 26, psy=1, t8=True, lo=26, hi=26) == (26, False, [26, 26], [])
    # nothing coded: the jump is clipped onto orig_qp itself
    assert run({26: (100, True)}, 26, 26, t8=True, lo=26, hi=26) == (26, False, [26, 26, 26], [])


def test_transform_flip_kept_and_undone():
    curve = {26: 100, 27: 110, 25: 90, 24: 80, 23: 85}
    assert run(curve, 26, 26, t8=True, flip_cost={24: 79}) == (24, True, [26, 27, 25, 24, 23, 26], [24])
    assert run(curve, 26, 26, t8=True, flip_cost={24: 80}) == (24, True, [26, 27, 25, 24, 23, 26], [24])          # undone only when it costs MORE
    assert run(curve, 26, 26, t8=True, flip_cost={24: 81}) == (24, False, [26, 27, 25, 24, 23, 26], [24])
    # the quantiser stays: the transform size is not asked about again
    assert run({26: 100, 27: 100, 25: 100}, 26, 26, t8=True, flip_cost={}) == (26, False, [26, 27, 25, 26], [])


def test_the_walk_chooses_inside_the_range_only():
    # a last_qp outside the range is not tried, however cheap (the walk down towards it tolerates one failure: 25, 24)
    assert run({26: 100, 27: 101, 25: 101, 24: 102, 10: 1}, 26, 10, lo=20, hi=30) == (26, False, [26, 27, 25, 24], [])
    # a macroblock whose own quantiser lies outside is left alone: nothing is asked
    assert run({}, 18, 26, lo=20, hi=30, t8=True) == (18, False, [], [])
    assert run({}, 31, 31, psy=1, lo=20, hi=30) == (31, False, [], [])
    # ... so the twin's guard (OutOfRange on any other quantiser) never fires: a curve that improves without end in both directions stops at the walls
    qp, flip, asked = R.walk(lambda q, f: (abs(q - 26) * -1 + 100, False), 26, 26, 20, 30, 0, False)
    assert [q for q, _ in asked] == [26, 27, 28, 29, 30, 25, 24, 23, 22, 21, 20, 26] and qp == 20


# ---- the host's rules (host/settings.cpp): --subme 10 under X264GPU_QP_RD=1, over the stand-in device ----
import json          # noqa: E402
import os            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

import settings_sessions as SS          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SUBME, TRELLIS, AQ = 28, 29, 40          # run_host_calls.PARAM_FIELDS: analyse.i_subpel_refine, analyse.i_trellis, rc.i_aq_mode
QPRD = dict(SS.CRF, subme=10, trellis=2, me="umh", **{"aq-mode": 1})          # a session that meets every condition


def _open(tmp_path, opts, qp_rd=True, n=2):
    env = {k: v for k, v in os.environ.items() if k not in SS.ENV_VARS + ("X264GPU_QP_RD",)}
    env.update(X264GPU_STUB_DEVICES="1", **({"X264GPU_QP_RD": "1"} if qp_rd else {}))
    args = [sys.executable, os.path.join(HERE, "stub", "run_host_calls.py"), "64", "48", str(n), "5"] + [k if v is None else f"{k}={v}" for k, v in opts.items()]
    out = subprocess.run(args, env=env, cwd=str(tmp_path), capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode().strip().splitlines()[-1])
    return got["params"], [(lvl, text) for lvl, text in got["log"] if "subme" in text]


def test_settings_subme_10_stays_with_the_variable_and_every_condition(tmp_path):
    params, lines = _open(tmp_path, QPRD)
    assert params[SUBME] == 10 and params[TRELLIS] == 2 and params[AQ] == 1 and lines == []
    params, lines = _open(tmp_path, dict(QPRD, subme=11, me="hex"))
    assert params[SUBME] == 10 and len(lines) == 1 and lines[0][0] == 2 and "full RD without early termination" in lines[0][1] and "subme 10" in lines[0][1]


@pytest.mark.parametrize("over,final,level,words", [
    ({"trellis": 1}, 9, 1, ("requires trellis 2 and aq-mode > 0", "x264", "trellis 2 missing")),          # x264's own two conditions, worded as its rule
    ({"aq-mode": 0}, 9, 1, ("requires trellis 2 and aq-mode > 0", "x264", "aq-mode > 0 missing")),
    ({"crf": None, "qp": 26}, 9, 1, ("requires trellis 2 and aq-mode > 0", "aq-mode > 0 missing")),         # a constant quantiser switches AQ off
    ({"no-cabac": None}, 7, 1, ("QP-RD", "needs CABAC", "subme 9")),                                          # (the refinement levels need CABAC too: on to 7)
    ({"me": "dia"}, 7, 1, ("QP-RD", "needs me hex / umh", "subme 9")),
    ({"psy-rd": "1.0:0.25"}, 9, 2, ("QP-RD is not run beside psy-trellis", "subme 9")),                      # psy-trellis keeps its kernels (and so does --nr, which the
                                                                                                              # stand-in device does not have: tests/test_gpu_qprd.py)
])
def test_settings_each_missing_condition_gives_subme_9_and_its_line(tmp_path, over, final, level, words):
    opts = {k: v for k, v in dict(QPRD, **over).items() if not (k == "crf" and "qp" in over)}
    params, lines = _open(tmp_path, opts)
    mine = [(lvl, t) for lvl, t in lines if "subme 10" in t]
    assert params[SUBME] == final and len(mine) == 1 and mine[0][0] == level and all(w in mine[0][1] for w in words), (params[SUBME], lines)


def test_settings_without_the_variable_nothing_changes(tmp_path):
    gold = json.load(open(os.path.join(HERE, "golden", "settings_parent_sessions.json")))
    for name in ("subme_10", "subme_11"):
        d = tmp_path / name
        d.mkdir()
        env_had = os.environ.pop("X264GPU_QP_RD", None)
        try:
            got = SS.run(name, str(d))
        finally:
            if env_had is not None:
                os.environ["X264GPU_QP_RD"] = env_had
        assert got == gold[name], name
    # ... and the session that would run QP-RD is the subme 9 one, with today's warning
    params, lines = _open(tmp_path, QPRD, qp_rd=False)
    assert params[SUBME] == 9 and [lvl for lvl, _ in lines] == [1] and "not implemented yet: subme 9" in lines[0][1]
