"""The label columns of include/dgdm_hip.h (dgdm_guidance_label / dgdm_guidance_label_settled) in numpy, from a tally or from final
poses.  Takes nothing computed by the code under test's reductions: its inputs are what Guidance.score / Guidance.rollout return."""
import numpy as np

TALLY, SETTLED = 10, 5


def tally_block(counts, sums, n_cells):
    """counts (M', 3, 3, 3) integer histograms and sums (M', 4) float32 of the block's objects -> the 10 tally columns, float32."""
    c = np.asarray(counts).reshape(-1, 3, 3, 3).astype(np.int64)
    s = np.asarray(sums, dtype=np.float32).reshape(-1, 4)
    den = np.float64(c.shape[0] * int(n_cells))
    k = [c[:, 0].sum(), c[:, 2].sum(), c[:, :, 0].sum(), c[:, :, 2].sum(), c[:, :, :, 0].sum(), c[:, :, :, 2].sum()]
    out = [np.float32(np.float64(int(v)) / den) for v in k]
    for j in range(4):
        acc = np.float64(0.0)
        for m in range(s.shape[0]):            # m ascending
            acc = acc + np.float64(s[m, j])
        out.append(np.float32(acc / den))
    return np.array(out, dtype=np.float32)


def tally_rows(counts, sums, n_cells, layout):
    """counts (M, B, 3, 3, 3), sums (M, B, 4) as Guidance.score returns them -> (B, 10) ('mean') or (B, M, 10) ('per_object')."""
    counts, sums = np.asarray(counts), np.asarray(sums)
    M, B = counts.shape[:2]
    if layout == "mean":
        return np.stack([tally_block(counts[:, b], sums[:, b], n_cells) for b in range(B)])
    return np.stack([np.stack([tally_block(counts[m:m + 1, b], sums[m:m + 1, b], n_cells) for m in range(M)]) for b in range(B)])


def settled_object(final, left):
    """final (G, 3) float64 = (ori, pos_x, pos_y) of one (object, finger) over g ascending, left (G,) -> (rho, c, s, p, fl, bad) in float64."""
    f = np.asarray(final, dtype=np.float64).reshape(-1, 3)
    G = f.shape[0]
    c = s = p = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            theta = np.float64(np.pi) * (f[g, 0] + np.float64(1.0))
            c = c + np.cos(theta)
            s = s + np.sin(theta)
            p = p + np.sqrt(f[g, 1] * f[g, 1] + f[g, 2] * f[g, 2])
        c, s, p = c / np.float64(G), s / np.float64(G), p / np.float64(G)
        rho = np.sqrt(c * c + s * s)
    fl = np.float64(int(np.count_nonzero(np.asarray(left).reshape(-1) >= 0))) / np.float64(G)
    return np.array([rho, c, s, p, fl], dtype=np.float64), not bool(np.isfinite(f).all())


def settled_block(finals, lefts):
    """finals (M', G, 3), lefts (M', G) of the block's objects -> the 5 settled columns, float32 (columns 0-3 NaN on a non-finite state)."""
    vals, bad = np.zeros(5, dtype=np.float64), False
    for m in range(len(finals)):               # m ascending
        v, b = settled_object(finals[m], lefts[m])
        with np.errstate(invalid="ignore", over="ignore"):
            vals = vals + v
        bad = bad or b
    with np.errstate(invalid="ignore", over="ignore"):
        out = (vals / np.float64(len(finals))).astype(np.float32)
    if bad:
        out[:4] = np.nan
    return out


def settled_rows(final, left, B, layout):
    """final (M, B*G, 3) float64 and left (M, B*G) as Guidance.rollout returns them (row = g*B + b) -> (B, 5) or (B, M, 5)."""
    final, left = np.asarray(final, dtype=np.float64), np.asarray(left)
    M = final.shape[0]
    f = final.reshape(M, -1, B, 3)             # (M, G, B, 3)
    l = left.reshape(M, -1, B)
    if layout == "mean":
        return np.stack([settled_block(f[:, :, b], l[:, :, b]) for b in range(B)])
    return np.stack([np.stack([settled_block(f[m:m + 1, :, b], l[m:m + 1, :, b]) for m in range(M)]) for b in range(B)])
