"""numpy float64 statement of synthsr_seg_resample_argmax (include/synthsr_hip.h), shared by tests/test_seg_native_cpu.py and
tests/test_seg_native_gpu.py: positions in float64, the inside rule, the clamped corner indices of
volumes.resample_volume_like, the weights rounded to float32 as the header says, everything after that in float64."""
import numpy as np

BOUNDARY_EPS = 1e-9    # a position this close to lo - 0.5 or hi + 0.5 may fall on either side on the device


def softmax_posteriors(shape, N, seed, sigma=3.0):
    """float32 [*shape, N]: the softmax of N(0, sigma^2) logits"""
    z = np.random.default_rng(seed).normal(0.0, sigma, size=tuple(shape) + (N,))
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def resample_argmax(probs, box, M, out_shape, labels, fill_value):
    """dict: 'probs' float64 [*out_shape, N] (0 outside), 'label' int32 [*out_shape], 'inside' bool, 'margin' float64 (largest
    minus second largest interpolated posterior; inf outside), 'near_boundary': the number of voxels with a coordinate within
    BOUNDARY_EPS of an inside / outside boundary"""
    probs = np.asarray(probs, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)[:3]
    lo, hi = np.asarray(box[:3], dtype=np.int64), np.asarray(box[3:], dtype=np.int64)
    N = probs.shape[3]
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing='ij')
    inside = np.ones(tuple(out_shape), dtype=bool)
    near = np.zeros(tuple(out_shape), dtype=bool)
    idx, wgt = [], []
    for a in range(3):
        pos = M[a, 0] * i + M[a, 1] * j + M[a, 2] * k + M[a, 3]
        inside &= (pos >= lo[a] - 0.5) & (pos <= hi[a] + 0.5)
        near |= (np.abs(pos - (lo[a] - 0.5)) < BOUNDARY_EPS) | (np.abs(pos - (hi[a] + 0.5)) < BOUNDARY_EPS)
        pos = np.clip(pos, lo[a], hi[a])
        i0 = np.minimum(np.floor(pos).astype(np.int64), max(hi[a] - 1, lo[a]))
        i1 = np.minimum(i0 + 1, hi[a])
        idx.append((i0, i1))
        wgt.append((pos - i0).astype(np.float32).astype(np.float64))
    p = np.zeros(tuple(out_shape) + (N,), dtype=np.float64)
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                w = ((wgt[0] if cz else 1.0 - wgt[0]) * (wgt[1] if cy else 1.0 - wgt[1]) * (wgt[2] if cx else 1.0 - wgt[2]))
                p += w[..., None] * probs[idx[0][cz], idx[1][cy], idx[2][cx]]
    p[~inside] = 0.0
    best = np.argmax(p, axis=-1)                      # the first of equal values: the lowest channel
    label = np.where(inside, np.asarray(labels, dtype=np.int64)[best], int(fill_value)).astype(np.int32)
    top = np.sort(p, axis=-1)
    margin = np.where(inside, top[..., -1] - top[..., -2], np.inf)
    return dict(probs=p, label=label, inside=inside, margin=margin, near_boundary=int(near.sum()), index=idx, weight=wgt)
