#!/usr/bin/env python3
"""A multipass encode through DriverProc (encoding type 4 of the config dialog: pass 1, then pass 2 without "update stats") in a process of its own, so that
X264GPU_MBTREE_STATS comes from the caller's environment (tests/test_gpu_mbtree_stats.py sets it).  The encode runs twice: in DIR/tree as the environment says,
then in DIR/plain with the variable taken out of this process' environment (the sessions read it when they open) — the tree-less encode of the commit before.
Usage: vfw_mbtree_child.py DIR W H FRAMES KBPS   -> one JSON line: per encode the two logs, the rate of the second pass' stream, what lies in its directory"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
for k in ("X264_HOST_STUB", "X264GPU_HOST_LIB", "X264GPU_LIB"):
    os.environ.pop(k, None)
import host_lib as V  # noqa: E402
from synth import synth_frames  # noqa: E402

D = V.H.DriverProc


def main():
    d = sys.argv[1]
    w, h, nfr, kbps = (int(x) for x in sys.argv[2:6])
    frames = synth_frames(w, h, nfr, seed=11, scene_len=53)

    def run(stats, i_pass, out, **fields):
        ico = V.ICOPEN(fccType=V.fourcc(b"vidc"))
        cid = D(0, None, V.DRV_OPEN, 0, V.addr(ico))
        n = D(cid, None, V.ICM_GETSTATE, 0, 0)
        cfg = V.VfwConfig()
        D(cid, None, V.ICM_GETSTATE, V.addr(cfg), n)
        cfg.i_encoding_type, cfg.i_passbitrate, cfg.i_pass, cfg.i_log_level = 4, kbps, i_pass, 3
        for k, v in fields.items():
            setattr(cfg, k, v)
        cfg.stats, cfg.i_output_mode, cfg.output_file = stats.encode(), 1, out.encode()
        cfg.extra_cmdline = b"--keyint 40 --rc-lookahead 8"
        D(cid, None, V.ICM_SETSTATE, V.addr(cfg), n)
        inb, outb = V.bmi(w, h, b"I420"), V.BITMAPINFO()
        assert D(cid, None, V.ICM_COMPRESS_GET_FORMAT, V.addr(inb), V.addr(outb)) == V.ICERR_OK
        assert D(cid, None, V.ICM_COMPRESS_BEGIN, V.addr(inb), V.addr(outb)) == V.ICERR_OK, V.H.x264vfw_shim_log(cid)
        cap = outb.bmiHeader.biSizeImage
        buf = C.create_string_buffer(cap)
        for f in frames:
            flags = V.DWORD(0)
            outb.bmiHeader.biSizeImage = cap
            icc = V.ICCOMPRESS(lpbiOutput=C.pointer(outb.bmiHeader), lpOutput=C.cast(buf, C.c_void_p), lpbiInput=C.pointer(inb.bmiHeader),
                               lpInput=f.ctypes.data, lpdwFlags=C.pointer(flags))
            assert D(cid, None, V.ICM_COMPRESS, V.addr(icc), C.sizeof(icc)) == V.ICERR_OK, V.H.x264vfw_shim_log(cid)
        log = V.H.x264vfw_shim_log(cid)
        assert D(cid, None, V.ICM_COMPRESS_END, 0, 0) == V.ICERR_OK
        D(cid, None, V.DRV_CLOSE, 0, 0)
        return log.decode(errors="replace")

    def encode(sub):
        os.mkdir(sub)
        stats = os.path.join(sub, "stats")
        log1 = run(stats, 1, os.path.join(sub, "p1.h264"))
        after1 = sorted(os.listdir(sub))
        log2 = run(stats, 2, os.path.join(sub, "p2.h264"), b_updatestats=0)
        size = os.path.getsize(os.path.join(sub, "p2.h264"))
        return {"log1": log1, "log2": log2, "after_pass1": after1, "files": sorted(os.listdir(sub)), "rate": size * 8 / (nfr / 25.0) / 1000.0}

    tree = encode(os.path.join(d, "tree"))
    os.environ.pop("X264GPU_MBTREE_STATS", None)
    plain = encode(os.path.join(d, "plain"))
    print(json.dumps({"tree": tree, "plain": plain}))


if __name__ == "__main__":
    main()
