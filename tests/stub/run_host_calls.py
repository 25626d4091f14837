#!/usr/bin/env python3
"""A session through x264_encoder_encode() of the STUB-backed host library, recorded call by call: the return value of every x264_encoder_encode (zeros and
errors included), x264_encoder_delayed_frames after every call, the formatted log at info level and above, the stream's SHA-256, the hash of what run_host.py
calls `meta`, and `params`: the x264_param_t fields the session's open rules touch as x264_encoder_parameters reports them right after the open (PARAM_FIELDS, in
that order), then x264host_pictures_in_flight.  The pictures, then flush calls while pictures are delayed, then one more flush call (a drained session answers 0).  late=K submits one more
picture after the K-th flush call, which a GOP-slot session refuses.  Prints one JSON line; tests/golden/gop_slots_parent_calls.json holds these lines as the
commit before host/gopslots.cpp printed them, tests/golden/settings_parent_sessions.json as the commit before host/settings.cpp did.  Usage: run_host_calls.py W H FRAMES SEED [late=K] key=value ...  (env X264GPU_STUB_DEVICES as run_host.py)"""
import ctypes as C
import hashlib
import json
import os
import sys

os.environ["X264_HOST_STUB"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import host_lib as HL  # noqa: E402
from quality_sessions import make_logger  # noqa: E402
from synth import synth_frames  # noqa: E402


# what x264_encoder_open's rules may change of the caller's parameters
PARAM_FIELDS = ("i_threads", "b_sliced_threads", "i_slice_count", "i_frame_reference", "i_keyint_max", "i_keyint_min", "i_scenecut_threshold",
                "i_bframe", "i_bframe_adaptive", "i_bframe_pyramid", "b_open_gop", "b_cabac", "i_cabac_init_idc", "b_interlaced", "b_constrained_intra",
                "b_intra_refresh", "i_level_idc", "i_nal_hrd", "analyse.inter", "analyse.intra", "analyse.b_transform_8x8", "analyse.i_weighted_pred",
                "analyse.b_weighted_bipred", "analyse.i_direct_mv_pred", "analyse.i_chroma_qp_offset", "analyse.i_me_method", "analyse.i_me_range",
                "analyse.i_mv_range", "analyse.i_subpel_refine", "analyse.i_trellis", "analyse.f_psy_rd", "analyse.f_psy_trellis", "analyse.i_noise_reduction",
                "analyse.b_mixed_references", "rc.i_rc_method", "rc.i_qp_constant", "rc.i_qp_min", "rc.i_qp_max", "rc.i_lookahead", "rc.b_mb_tree", "rc.i_aq_mode",
                "rc.i_vbv_max_bitrate", "rc.i_vbv_buffer_size", "rc.f_vbv_buffer_init", "rc.b_stat_read", "rc.b_stat_write", "i_slice_max_size", "i_slice_max_mbs",
                "b_fake_interlaced", "b_pic_struct", "b_bluray_compat")


def reported_params(H, h_):
    q = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(q))
    vals = []
    for name in PARAM_FIELDS:
        v = q
        for part in name.split("."):
            v = getattr(v, part)
        vals.append(round(v, 6) if isinstance(v, float) else int(v))
    return vals + [int(H.x264host_pictures_in_flight(h_))]


def session(w, h, n, seed, opts, late=None, preset=b"medium"):
    H = HL.H
    frames = synth_frames(w, h, n + 1, seed=seed)
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_
    params = reported_params(H, h_)
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    planes = [(w * h, 0), (w * h // 4, w * h), (w * h // 4, w * h * 5 // 4)]
    stream, meta, rets, delayed = b"", [], [], []

    def call(i):          # picture i, or a flush call (None)
        nonlocal stream
        if i is not None:
            for pl, (sz, off) in enumerate(planes):
                C.memmove(pic.img.plane[pl], frames[i][off:off + sz].ctypes.data, sz)
            pic.i_pts = i
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None if i is None else C.byref(pic), C.byref(out))
        rets.append(size)
        delayed.append(H.x264_encoder_delayed_frames(h_))
        if size > 0:
            stream += C.string_at(nal[0].p_payload, size)
            meta.append((int(out.i_type), int(out.b_keyframe), int(out.i_pts), int(out.i_dts), [(int(nal[k].i_type), int(nal[k].i_ref_idc)) for k in range(nn.value)]))
    for i in range(n):
        call(i)
    flushes = 0
    while H.x264_encoder_delayed_frames(h_) and flushes < n + 8:
        call(None)
        flushes += 1
        if late == flushes: call(n)
    call(None)
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return {"rets": rets, "delayed": delayed, "log": [[lvl, text] for lvl, text in log], "sha": hashlib.sha256(stream).hexdigest(),
            "meta": hashlib.sha256(json.dumps(meta).encode()).hexdigest(), "params": params}


if __name__ == "__main__":
    w, h, n, seed = (int(x) for x in sys.argv[1:5])
    opts = {}
    for a in sys.argv[5:]:
        k, eq, v = a.partition("=")
        opts[k] = v if eq else None
    late = opts.pop("late", None)
    print(json.dumps(session(w, h, n, seed, opts, None if late is None else int(late))))
