"""Time per pass of eight blocks of the trellis primitive (csrc/trellis.hip.h through x264gpu_trellis_blocks_ex): the automatic choice of loop beside the
forced general loop, at the bench's quantisers (20 intra; 23, 24, 25 inter), on a dense input (Laplacian amplitudes of a few steps) and on a sparse
one whose every guess is 0 or 1.  One wavefront runs the passes one after the other, so time / passes is the latency of a call."""
import sys, time
import os; R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np, torch
from x264vfw_amd import lib
rng = np.random.default_rng(1)
nblk = 8000
Q4MAX, Q8MAX = [13107, 11916, 10082, 9362, 8192, 7282], [20972, 19174, 15978, 14913, 13159, 11570]
print("cat qp intra input   auto_us forced_us  speedup  ones%  nonzero/blk")
for cat, nc in ((2, 16), (5, 64), (4, 16), (3, 4)):
    for qp, intra in ((20, 1), (23, 0), (24, 0), (25, 0)):
        # the smallest quantiser step among the block's coefficient classes (65536 / the largest mf of the row)
        srd = lambda x, s: x << -s if s <= 0 else (x + (1 << (s - 1))) >> s
        mf_max = srd(Q8MAX[qp % 6], qp // 6) if cat == 5 else srd(Q4MAX[qp % 6], qp // 6 - 1) >> (1 if cat == 3 else 0)
        step = 65536.0 / mf_max
        for name in ("dense", "sparse"):
            if name == "dense":
                amp = step * 6.0 / (1.0 + 0.35 * np.arange(nc))
                coefs = (rng.laplace(0, 1, (nblk, nc)) * amp).astype(np.int16)
            else:
                # +-1.1 of the smallest step (a guess of 1 there, of 1 or 0 in the coarser classes), about four per block
                coefs = (np.round(step * 1.1) * rng.choice([-1, 1], (nblk, nc)) * (rng.random((nblk, nc)) < 4.0 / nc)).astype(np.int16)
            if cat == 4: coefs[:, 0] = 0
            states = ((rng.integers(0, 63, 460) << 1) | rng.integers(0, 2, 460)).astype(np.uint8)
            d_c, d_s = torch.from_numpy(coefs).cuda(), torch.from_numpy(states).cuda()
            d_l, d_z = torch.zeros_like(d_c), torch.zeros(nblk, dtype=torch.uint8, device='cuda')
            d_p = torch.zeros(nblk // 8, dtype=torch.uint8, device='cuda')
            us = []
            for force in (0, 1):
                for it in range(3):
                    torch.cuda.synchronize(); t0 = time.time()
                    lib.check(lib.x264gpu_trellis_blocks_ex(d_c.data_ptr(), nblk, cat, qp, intra, d_s.data_ptr(), d_l.data_ptr(), d_z.data_ptr(), force, d_p.data_ptr() if not force else None, None), "t")
                    torch.cuda.synchronize(); dt = time.time() - t0
                us.append(dt * 1e6 / (nblk / 8))
            p = d_p.cpu().numpy()
            nnz = np.count_nonzero(d_l.cpu().numpy()) / nblk
            print(f"{cat:3d} {qp:2d} {intra:5d} {name:6s} {us[0]:8.2f} {us[1]:9.2f} {us[1] / us[0]:8.2f} {100.0 * np.mean(p & 1):6.1f} {nnz:8.1f}")
