"""CPU oracle of the icon-contour contract (DESIGN.md "Object contours from icon images"): the reference's
assets/icon_process.py:extract_contours (cv2.resize to 128 x 128, BGR2GRAY, threshold 240 inverted, external contours with
CHAIN_APPROX_SIMPLE, the longest by arcLength, resample_contour, int32, rescale) written out step by step in numpy and plain Python.
Test infrastructure only: tests/test_icon_oracle.py checks it against known answers, tests/test_gpu_icon_contours.py holds
csrc/contour.hip to it bit for bit."""
import math

import numpy as np

SIZE = 128
DX = (1, 1, 0, -1, -1, -1, 0, 1)         # direction s: (DX[s], DY[s]), y pointing down
DY = (0, -1, -1, -1, 0, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ resize
def linear_taps(src: int, dst: int = SIZE):
    """Per output index: (source index, weight of it, weight of the next one), the fixed-point INTER_LINEAR table."""
    scale = 1.0 / (float(dst) / float(src))         # OpenCV: inv_scale = dst / src, scale = 1 / inv_scale
    sx, w0, w1 = [], [], []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0.0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0.0)
        sx.append(s)
        w0.append(int(np.rint(np.float32(np.float32(1.0) - f) * np.float32(2048))))
        w1.append(int(np.rint(f * np.float32(2048))))
    return np.array(sx, dtype=np.int64), np.array(w0, dtype=np.int64), np.array(w1, dtype=np.int64)


def resize(img: np.ndarray) -> np.ndarray:
    """(H, W, C) uint8 -> (128, 128, C) uint8, per channel."""
    H, W = img.shape[:2]
    S = img.astype(np.int64)
    if H == SIZE and W == SIZE:
        return img.copy()
    if H == 2 * SIZE and W == 2 * SIZE:                 # INTER_LINEAR at an exact factor of 2 is OpenCV's area path
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = linear_taps(W)
    sy, b0, b1 = linear_taps(H)
    sx1 = np.minimum(sx + 1, W - 1)
    sy1 = np.minimum(sy + 1, H - 1)
    hr = S[:, sx] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]          # horizontal pass, (H, 128, C)
    h0, h1 = hr[sy] >> 4, hr[sy1] >> 4
    v = (((h0 * b0[:, None, None]) >> 16) + ((h1 * b1[:, None, None]) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_scalar(img: np.ndarray) -> np.ndarray:
    """OpenCV's scalar vertical pass (b0 h0 + b1 h1 + 2^21) >> 22, which the contract does NOT use."""
    H, W = img.shape[:2]
    S = img.astype(np.int64)
    sx, a0, a1 = linear_taps(W)
    sy, b0, b1 = linear_taps(H)
    hr = S[:, sx] * a0[None, :, None] + S[:, np.minimum(sx + 1, W - 1)] * a1[None, :, None]
    v = (hr[sy] * b0[:, None, None] + hr[np.minimum(sy + 1, H - 1)] * b1[:, None, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def grey(img: np.ndarray) -> np.ndarray:
    """BGR(A) uint8 -> Y uint8."""
    S = img.astype(np.int64)
    return ((1868 * S[..., 0] + 9617 * S[..., 1] + 4899 * S[..., 2] + 8192) >> 14).astype(np.uint8)


def foreground(img: np.ndarray) -> np.ndarray:
    """(H, W, 3|4) uint8 -> (128, 128) bool: THRESH_BINARY_INV at 240 of the grey resized image."""
    return grey(resize(img)) <= 240


# ------------------------------------------------------------------------------------------------------------------ contours
def _follow(lab, x0, y0, mark=True):
    """icvFetchContour of an outer border starting at framed (x0, y0), CHAIN_APPROX_SIMPLE; lab is the framed (130 x 130) label list.
    Returns the points in image coordinates."""
    W = SIZE + 2
    pts = []
    s = s_end = 4
    while True:
        s = (s - 1) & 7
        x1, y1 = x0 + DX[s], y0 + DY[s]
        if lab[y1 * W + x1] != 0 or s == s_end:
            break
    if s == s_end:                                  # no foreground neighbour: a one-point contour
        if mark:
            lab[y0 * W + x0] = -126
        return [(x0 - 1, y0 - 1)]
    x3, y3 = x0, y0
    prev_s = s ^ 4
    while True:
        s_end = s
        while True:                                 # counter-clockwise from s_end + 1; the pixel we came from ends it at the latest
            s += 1
            x4, y4 = x3 + DX[s & 7], y3 + DY[s & 7]
            if lab[y4 * W + x4] != 0:
                break
        s &= 7
        if mark:
            if 0 <= s - 1 < s_end:                  # the search passed direction 0 (right neighbour background)
                lab[y3 * W + x3] = -126
            elif lab[y3 * W + x3] == 1:
                lab[y3 * W + x3] = 2
        if s != prev_s:
            pts.append((x3 - 1, y3 - 1))
            prev_s = s
        if x4 == x0 and y4 == y0 and x3 == x1 and y3 == y1:
            break
        x3, y3 = x4, y4
        s = (s + 4) & 7
    return pts


def external_contours(mask: np.ndarray):
    """RETR_EXTERNAL + CHAIN_APPROX_SIMPLE on a (128, 128) bool mask framed by background: the outer borders in order of discovery
    (raster order of their start pixels), each a list of (x, y)."""
    W = SIZE + 2
    framed = np.zeros((W, W), dtype=np.int64)
    framed[1:-1, 1:-1] = np.asarray(mask, dtype=bool)
    lab = framed.reshape(-1).tolist()
    out = []
    for y in range(1, SIZE + 1):
        prev, lnbd = 0, 0                            # lnbd: the label of the last marked pixel passed on the row (column 0: frame)
        base = y * W
        for x in range(1, SIZE + 1):
            p = lab[base + x]
            if p == prev:
                continue
            if prev == 0 and p == 1:                 # outer border candidate
                if lnbd <= 0:
                    out.append(_follow(lab, x, y))
                    p = lab[base + x]
                    lnbd = p
                    prev = p
                    continue
            elif p == 0 and prev >= 1 and (prev & -2):   # hole border candidate (never traced): lnbd moves to its left pixel
                lnbd = prev
            if p & -2:
                lnbd = p
            prev = p
    return out


def arc_length(pts) -> float:
    """cv2.arcLength(closed=True) of int points: float32 segment lengths accumulated in double, closing segment first."""
    n = len(pts)
    if n <= 1:
        return 0.0
    total = 0.0
    px, py = pts[-1]
    for x, y in pts:
        dx, dy = np.float32(x - px), np.float32(y - py)
        total += float(np.sqrt(np.float32(dx * dx + dy * dy)))
        px, py = x, y
    return total


def largest_contour(mask: np.ndarray):
    """The contour extract_contours keeps: the longest; on an exact tie the one discovered last (cv2 lists them newest first and
    np.argmax takes the first maximum).  None for an empty mask."""
    best, best_len = None, -1.0
    for c in external_contours(mask):
        ln = arc_length(c)
        if ln >= best_len:
            best, best_len = c, ln
    return best


# ------------------------------------------------------------------------------------------------------------------ resample
def interp(u: float, c: np.ndarray, fp: np.ndarray) -> float:
    """np.interp at one point for non-decreasing c (no FMA: two roundings)."""
    K = len(c)
    if K == 1:
        return float(fp[0])
    j = int(np.searchsorted(c, u, side="right")) - 1
    if j >= K - 1 or c[j] == u:
        return float(fp[min(j, K - 1)])
    slope = (float(fp[j + 1]) - float(fp[j])) / (float(c[j + 1]) - float(c[j]))
    return slope * (u - float(c[j])) + float(fp[j])


def resample(points, n: int) -> np.ndarray:
    """resample_contour written out: (K, 2) int -> (n, 2) int32."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    K = len(p)
    c = np.zeros(K, dtype=np.float64)
    for i in range(1, K):
        d = p[i] - p[i - 1]
        c[i] = c[i - 1] + math.sqrt(float(d[0] * d[0] + d[1] * d[1]))
    L = float(c[K - 1])
    if n == 1:
        u = [0.0]
    else:
        step = L / (n - 1)
        u = [j * step for j in range(n)] if step != 0 else [0.0] * n
        u[-1] = L
    out = np.empty((n, 2), dtype=np.int32)
    for j, uj in enumerate(u):
        out[j, 0] = int(interp(uj, c, p[:, 0]))      # int(): truncation toward zero, as astype(np.int32)
        out[j, 1] = int(interp(uj, c, p[:, 1]))
    return out


def rescale(c: np.ndarray) -> np.ndarray:
    return c / 128 * 0.1 - 0.05


def extract(image: np.ndarray, num_points: int = 100, rescaled: bool = True) -> np.ndarray:
    """extract_contours of one (H, W, 3|4) uint8 image."""
    best = largest_contour(foreground(image))
    if best is None:
        raise ValueError("no foreground pixel")
    r = resample(best, num_points)
    return rescale(r) if rescaled else r
