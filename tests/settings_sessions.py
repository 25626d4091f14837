"""The sessions behind tests/golden/settings_parent_sessions.json: one row for every rule x264_encoder_open applies to the caller's parameters (host/settings.cpp),
both ways where a rule has two.  A row is (pictures, options, environment, first pass or None, width x height); tests/stub/run_host_calls.py runs it over the
stand-in device in a directory of its own (statistics files are named relative to it), a row with a first pass after that pass has run there.
`python tests/settings_sessions.py > tests/golden/settings_parent_sessions.json` records every row; it was run on the commit before host/settings.cpp existed."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("rets", "delayed", "log", "sha", "meta", "params")
ENV_VARS = ("X264GPU_BATCH", "X264GPU_GOP_SLOTS", "X264GPU_GOP_SLOTS_RC", "X264GPU_INFLIGHT", "X264GPU_DUMP_RECORDS", "X264GPU_HOST_PIPELINE",
            "X264GPU_CAVLC_THREADS", "X264GPU_MBTREE_STATS", "X264GPU_DEVICES")

# I / P pictures at a constant quantiser, nothing held back: the session the toolset rules are shown on
IP = {"qp": 30, "keyint": 8, "scenecut": 0, "bframes": 0, "weightp": 0, "rc-lookahead": 0}
# ... with B pictures (on the DPB model)
B = {"qp": 30, "keyint": 8, "scenecut": 0, "bframes": 2, "b-adapt": 0, "weightp": 0, "rc-lookahead": 0}
CRF = {"crf": 26, "keyint": 8, "scenecut": 0, "bframes": 0, "weightp": 0, "rc-lookahead": 0, "no-mbtree": None}
CRFB = dict(CRF, bframes=2, **{"b-adapt": 0})
ABR = {"bitrate": 300, "keyint": 8, "scenecut": 0, "bframes": 0, "weightp": 0, "rc-lookahead": 0, "no-mbtree": None}
VBV = {"vbv-maxrate": 500, "vbv-bufsize": 500}
PASS = dict(ABR, bframes=2, **{"b-adapt": 0}, stats="s.stats")
TREE = {"mbtree": None, "rc-lookahead": 5}
BATCH = {"X264GPU_BATCH": "2"}
SMALL, TALL = (64, 48), (64, 128)


def _drop(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def row(n, opts, env=None, first=None, size=SMALL):
    return (n, opts, env or {}, first, size)


SESSIONS = {
    # ---- toolset ----
    "ref_8": row(3, dict(IP, ref=8)),
    "cabac_idc": row(3, dict(IP, **{"cabac-idc": 2})),
    "p4x4": row(3, dict(IP, partitions="all")),
    "tesa": row(3, dict(IP, me="tesa")),
    "subme_10": row(3, dict(IP, subme=10)),
    "subme_11": row(3, dict(IP, subme=11)),
    "subme_8": row(3, dict(IP, subme=8)),
    "subme_8_cavlc": row(3, dict(IP, subme=8, **{"no-cabac": None})),
    "subme_8_dia": row(3, dict(IP, subme=8, me="dia")),
    "subme_8_esa": row(3, dict(IP, subme=8, me="esa")),
    "trellis_cavlc": row(3, dict(IP, trellis=1, **{"no-cabac": None})),
    "trellis_subme_5": row(3, dict(IP, trellis=2, subme=5)),
    "psy_trellis_cavlc": row(3, dict(IP, trellis=1, **{"psy-rd": "1.0:0.5", "no-cabac": None})),
    "psy_trellis_subme_5": row(3, dict(IP, trellis=1, subme=5, **{"psy-rd": "1.0:0.5"})),
    "psy_trellis_dia": row(3, dict(IP, trellis=1, me="dia", **{"psy-rd": "1.0:0.5"})),
    "psy_trellis_without_trellis": row(3, dict(IP, trellis=0, **{"psy-rd": "1.0:0.5"})),
    "psy_both_low": row(3, dict(IP, trellis=1, **{"psy-rd": "0.2:0.2"})),
    "psy_both_high": row(3, dict(IP, trellis=1, **{"psy-rd": "1.0:0.5"})),
    "psy_trellis_alone": row(3, dict(IP, trellis=1, **{"psy-rd": "0:0.5"})),
    "no_psy": row(3, dict(IP, trellis=1, **{"psy-rd": "1.0:0.5", "no-psy": None})),
    "interlaced_constrained_refresh": row(3, dict(IP, **{"interlaced": None, "constrained-intra": None, "intra-refresh": None})),
    "sliced_threads_too_many": row(3, dict(IP, threads=4, slices=3, **{"sliced-threads": None}), size=TALL),
    "sliced_threads_one_slice": row(3, dict(IP, threads=4, **{"sliced-threads": None})),
    "sliced_threads_gop_slots": row(10, dict(IP, keyint=4, threads=2, **{"sliced-threads": None, "min-keyint": 4}), {"X264GPU_GOP_SLOTS": "2"}, size=TALL),
    "slices_above_rows": row(3, dict(IP, slices=9)),
    "cavlc_threads_2": row(3, dict(IP, **{"no-cabac": None}), {"X264GPU_CAVLC_THREADS": "2"}),
    # ---- VBV and HRD ----
    "vbv_constant_quantiser": row(3, dict(B, **VBV)),
    "vbv_threads_2": row(3, dict(CRF, threads=2, **VBV)),
    "vbv_batch": row(3, dict(CRF, scenecut=40, **VBV), BATCH),
    "vbv_second_pass": row(3, dict(ABR, **{"pass": 2}, stats="s.stats", **VBV)),
    "vbv_bufsize_alone_crf": row(3, dict(CRF, **{"vbv-bufsize": 500})),
    "vbv_bufsize_alone_abr": row(3, dict(ABR, **{"vbv-bufsize": 300})),
    "vbv_maxrate_alone": row(3, dict(CRF, **{"vbv-maxrate": 500})),
    "vbv_maxrate_below_bitrate": row(3, dict(ABR, **{"vbv-maxrate": 200, "vbv-bufsize": 300})),
    "vbv_buffer_below_one_frame": row(3, dict(CRF, **{"vbv-maxrate": 1000, "vbv-bufsize": 10})),
    "vbv_init_kbit": row(3, dict(CRF, **VBV, **{"vbv-init": 250})),
    "vbv_lookahead": row(6, dict(CRFB, **VBV, **{"rc-lookahead": 3, "crf-max": 40})),
    "hrd_without_vbv": row(3, dict(CRF, **{"nal-hrd": "vbr"})),
    "hrd_cbr_under_crf": row(3, dict(CRF, **VBV, **{"nal-hrd": "cbr"})),
    "hrd_cbr": row(3, dict(ABR, **{"vbv-maxrate": 300, "vbv-bufsize": 300, "nal-hrd": "cbr"})),
    # ---- picture structure ----
    "b_crf_threads_2": row(3, dict(CRFB, threads=2)),
    "b_keyint_1": row(3, dict(B, keyint=1)),
    "b_abr_without_bitrate": row(3, dict(_drop(B, "qp"), bitrate=0)),
    "b_adapt_direct_auto_threads_2": row(9, dict(B, keyint=4, threads=2, direct="auto", **{"b-adapt": 1, "min-keyint": 4})),
    "b_pyramid_strict_open_gop_direct_none": row(5, dict(B, bframes=3, direct="none", **{"b-pyramid": "strict", "open-gop": None})),
    "b_one_without_pyramid": row(4, dict(B, bframes=1)),
    "direct_auto_batch": row(4, dict(B, direct="auto", **{"b-adapt": 1}), BATCH),
    "direct_auto": row(5, dict(B, direct="auto")),
    "weightp_1_without_b": row(3, dict(IP, weightp=1)),
    "weightp_1_with_b": row(4, dict(B, weightp=1)),
    "weightp_2_threads_2": row(9, dict(IP, keyint=4, weightp=2, threads=2, **{"min-keyint": 4})),
    "weightp_2_mbtree": row(4, dict(CRF, weightp=2, **TREE)),
    "weightp_2_abr_without_bitrate": row(3, dict(_drop(IP, "qp"), bitrate=0, weightp=2)),
    "weightp_2_keyint_1": row(3, dict(IP, weightp=2, keyint=1)),
    "weightp_2_ref_1": row(3, dict(IP, weightp=2, ref=1)),
    "weightp_2_without_b": row(4, dict(IP, weightp=2, ref=2)),
    "keyint_0": row(2, dict(IP, keyint=0)),
    # ---- X264GPU_BATCH: a session that may not join runs on its own ----
    "batch_threads_2": row(9, dict(IP, keyint=4, threads=2, **{"min-keyint": 4}), BATCH),
    "batch_slices": row(3, dict(IP, slices=2), BATCH),
    "batch_scenecut": row(3, dict(IP, scenecut=40), BATCH),
    "batch_b_adapt": row(4, dict(B, **{"b-adapt": 1}), BATCH),
    "batch_abr": row(3, ABR, BATCH),
    "batch_of_1": row(3, IP, {"X264GPU_BATCH": "1"}),
    # ---- rate control ----
    "pass_1": row(5, dict(PASS, **{"pass": 1})),
    "pass_2": row(5, dict(PASS, **{"pass": 2}), first=dict(PASS, **{"pass": 1})),
    "pass_1_off_the_dpb_model": row(3, dict(ABR, **{"pass": 1}, stats="s.stats")),
    "pass_3_off_the_dpb_model": row(3, dict(ABR, **{"pass": 3}, stats="s.stats")),
    "pass_1_batch": row(4, dict(PASS, scenecut=40, **{"pass": 1}), BATCH),
    "pass_1_mbtree_without_file": row(5, dict(_drop(PASS, "no-mbtree"), **TREE, **{"pass": 1})),
    "pass_1_mbtree_file": row(5, dict(_drop(PASS, "no-mbtree"), **TREE, **{"pass": 1}), {"X264GPU_MBTREE_STATS": "1"}),
    "pass_2_mbtree_file": row(5, dict(_drop(PASS, "no-mbtree"), **TREE, **{"pass": 2}), {"X264GPU_MBTREE_STATS": "1"}, first=dict(_drop(PASS, "no-mbtree"), **TREE, **{"pass": 1})),
    "zones": row(4, dict(CRF, zones="1,2,q=35")),
    "zones_two": row(4, dict(IP, zones="0,1,q=20/2,3,b=0.5")),
    "zones_second_pass": row(5, dict(PASS, zones="1,2,b=0.5", **{"pass": 2}), first=dict(PASS, **{"pass": 1})),
    "abr_threads_2": row(9, dict(ABR, keyint=4, threads=2, **{"min-keyint": 4})),
    "crf_threads_2_mbtree_scenecut": row(9, dict(_drop(CRF, "no-mbtree"), keyint=4, threads=2, scenecut=40, **TREE, **{"min-keyint": 4})),
    "lossless": row(2, dict(IP, qp=0)),
    "crf_below_1": row(2, dict(CRF, crf=0.5)),
    "qpmin_qpmax": row(3, dict(CRF, qpmin=60, qpmax=5)),
    # ---- noise reduction ----
    "nr_beside_psy_trellis": row(4, dict(B, nr=100, trellis=1, **{"psy-rd": "1.0:0.5"})),
    # ---- smaller rules ----
    "slice_max_fake_interlaced_bluray": row(3, dict(IP, **{"slice-max-size": 500, "fake-interlaced": None, "bluray-compat": None})),
    "aq_mode_2_off_the_dpb_model": row(3, dict(CRF, **{"aq-mode": 2})),
    "aq_mode_3_b": row(4, dict(CRFB, **{"aq-mode": 3})),
    "aq_strength_0": row(3, dict(CRF, **{"aq-strength": 0})),
    "min_keyint_given": row(3, dict(IP, **{"min-keyint": 3})),
    "min_keyint_above_half": row(3, dict(IP, **{"min-keyint": 7})),
    "mvrange_given": row(3, dict(IP, mvrange=16)),
    "level_given": row(3, dict(B, level="3.1")),
    "keyint_infinite_threads_2": row(3, dict(IP, keyint="infinite", threads=2)),
    # ---- lookahead and pictures in flight ----
    "lookahead_70_b": row(5, dict(_drop(CRFB, "no-mbtree"), keyint=250, mbtree=None, **{"rc-lookahead": 70})),
    "lookahead_window_widest": row(5, dict(_drop(CRFB, "no-mbtree"), keyint=250, bframes=16, ref=1, mbtree=None, **{"rc-lookahead": 70, "b-adapt": 2, "b-pyramid": "none"}),
                                   {"X264GPU_INFLIGHT": "9"}),
    "lookahead_above_keyint": row(5, dict(_drop(CRF, "no-mbtree"), mbtree=None, **{"rc-lookahead": 20})),
    "pipeline": row(6, dict(_drop(CRF, "no-mbtree"), mbtree=None, **{"rc-lookahead": 3})),
    "pipeline_off": row(6, dict(_drop(CRF, "no-mbtree"), mbtree=None, **{"rc-lookahead": 3}), {"X264GPU_HOST_PIPELINE": "0"}),
    "inflight_unset": row(7, CRFB),
    "inflight_1": row(7, CRFB, {"X264GPU_INFLIGHT": "1"}),
    "inflight_2": row(7, CRFB, {"X264GPU_INFLIGHT": "2"}),
    "inflight_9": row(7, CRFB, {"X264GPU_INFLIGHT": "9"}),
    "inflight_dump_records": row(4, CRFB, {"X264GPU_DUMP_RECORDS": "."}),
    "inflight_nr": row(4, dict(CRFB, nr=100, trellis=1), {"X264GPU_INFLIGHT": "2"}),
    "inflight_b_adapt_2": row(7, dict(CRFB, **{"b-adapt": 2})),
    "slots_rc": row(10, dict(CRFB, keyint=4, threads=2, **{"min-keyint": 4}), {"X264GPU_GOP_SLOTS_RC": "1"}),
    "slots_rc_mbtree": row(10, dict(_drop(CRFB, "no-mbtree"), keyint=4, threads=2, weightp=2, **TREE, **{"min-keyint": 4}), {"X264GPU_GOP_SLOTS_RC": "1"}),
    "slots_rc_vbv": row(10, dict(CRFB, keyint=4, threads=2, **VBV, **{"min-keyint": 4}), {"X264GPU_GOP_SLOTS_RC": "1"}),
    "slots_rc_keyint_infinite": row(4, dict(CRFB, keyint="infinite", threads=2), {"X264GPU_GOP_SLOTS_RC": "1"}),
}


def run(name, cwd):
    """tests/stub/run_host_calls.py's line for SESSIONS[name], run in directory `cwd` (empty before)"""
    n, opts, env_add, first, (w, h) = SESSIONS[name]
    env = {k: v for k, v in os.environ.items() if k not in ENV_VARS}
    env.update(env_add, X264GPU_STUB_DEVICES="1")
    got = None
    for o in ([first] if first else []) + [opts]:
        args = [sys.executable, os.path.join(HERE, "stub", "run_host_calls.py"), str(w), str(h), str(n), "5"] + [k if v is None else f"{k}={v}" for k, v in o.items()]
        out = subprocess.run(args, env=env, cwd=cwd, capture_output=True, timeout=600)
        assert out.returncode == 0, (name, out.stderr.decode()[-2000:])
        got = json.loads(out.stdout.decode().strip().splitlines()[-1])
    return {k: got[k] for k in KEYS}


if __name__ == "__main__":
    gold = {}
    for name in sorted(SESSIONS):
        with tempfile.TemporaryDirectory() as d:
            gold[name] = run(name, d)
    print(json.dumps(gold, separators=(",", ":"), sort_keys=True))
