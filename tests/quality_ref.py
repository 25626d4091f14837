"""numpy reference of the picture-quality statistics (include/x264gpu.h x264gpu_quality; x264's pixel_ssd_wxh, pixel_ssim_wxh, ssim_end1 for 8-bit
samples, restated): exact integer sums, the window values in float64."""
import numpy as np

C1, C2 = int(.01 * .01 * 255 * 255 * 64 + .5), int(.03 * .03 * 255 * 255 * 64 * 63 + .5)


def planes(i420, w, h):
    """(Y, U, V) of a tight I420 picture"""
    y = i420[:w * h].reshape(h, w)
    u = i420[w * h:w * h * 5 // 4].reshape(h // 2, w // 2)
    v = i420[w * h * 5 // 4:w * h * 3 // 2].reshape(h // 2, w // 2)
    return y, u, v


def ssd(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def ssim_windows(a, b):
    """luma planes -> the window values (float64), shape (zr - 1, zc - 1)"""
    h, w = a.shape
    zc, zr = (w - 2) >> 2, (h - 2) >> 2
    a = a[2:2 + 4 * zr, 2:2 + 4 * zc].astype(np.int64)
    b = b[2:2 + 4 * zr, 2:2 + 4 * zc].astype(np.int64)

    def blocks(x):          # sums over the 4x4 blocks, by reshape
        return x.reshape(zr, 4, zc, 4).sum(axis=(1, 3))

    def win(x):             # a window = a block and its right, lower and lower-right neighbours
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    s1, s2, ss, s12 = win(blocks(a)), win(blocks(b)), win(blocks(a * a + b * b)), win(blocks(a * b))
    assert max(int((2 * s1 * s2 + C1).max()), int((ss * 64).max())) < 2 ** 31          # x264 keeps these in 32-bit integers
    vars_ = ss * 64 - s1 * s1 - s2 * s2
    covar = s12 * 64 - s1 * s2
    return (2 * s1 * s2 + C1).astype(np.float64) * (2 * covar + C2).astype(np.float64) / ((s1 * s1 + s2 * s2 + C1).astype(np.float64) * (vars_ + C2).astype(np.float64))


def ssim_count(w, h):
    return (((w - 2) >> 2) - 1) * (((h - 2) >> 2) - 1)


def quality(a420, b420, w, h):
    """-> dict(ssd = [Y, U, V], ssim_sum, ssim_cnt, ssim) of two tight I420 pictures"""
    pa, pb = planes(a420, w, h), planes(b420, w, h)
    wv = ssim_windows(pa[0], pb[0])
    return dict(ssd=[ssd(x, y) for x, y in zip(pa, pb)], ssim_sum=float(wv.sum()), ssim_cnt=int(wv.size), ssim=float(wv.sum() / wv.size))


def psnr(sqe, n):
    mse = sqe / (255.0 * 255.0 * n)
    return 100.0 if mse <= 0.0000000001 else -10.0 * np.log10(mse)


def ssim_db(ssim):
    inv = 1.0 - ssim
    return 100.0 if inv <= 0.0000000001 else -10.0 * np.log10(inv)


def picture_psnr(s, w, h):
    """[Y, U, V, Avg] from the three sums of squared differences"""
    return [psnr(s[0], w * h), psnr(s[1], w * h / 4), psnr(s[2], w * h / 4), psnr(s[0] + s[1] + s[2], 3 * w * h / 2)]
