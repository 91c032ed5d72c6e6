"""Golden values of the two segmentation losses that synthsr_amd takes on the logits, from the reference's own layer code
executed through the numpy TF/Keras shim of this directory:

    ext/lab2im/layers.py:1408-1412   WeightedL2Loss.call      (target_value 5, the default, and 3)
    ext/lab2im/layers.py:1498-1526   CrossEntropyLoss.call    (enable_checks=False, no class or boundary weights)

One tiny case: a one-hot ground truth [1, 4, 5, 6, 5] with some all-zero rows (voxels without a class), random logits (what
WeightedL2Loss is fed) and random posteriors (what CrossEntropyLoss is fed).  Writes tests/golden/seg_losses.npz: the three
inputs and the scalars, data only.  Run from the repository root:  python tests/golden/gen/make_seg_losses_golden.py
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
REF = '/root/reference'
sys.path.insert(0, HERE)

import tf_numpy_shim as shim  # noqa: E402
import keras_layers_shim as ks  # noqa: E402

ks.install([], REF)
# the one op of CrossEntropyLoss.call that the shim's tensorflow.math lacks
sys.modules['tensorflow'].math.reduce_mean = sys.modules['tensorflow'].reduce_mean

from ext.lab2im import layers as l2i_layers  # noqa: E402


def main():
    rng = np.random.default_rng(20)
    shape, N = (1, 4, 5, 6), 5
    k = rng.integers(0, N, shape)
    k[0, 0, 0, :3] = 0                      # some background voxels for the 1e-8 weight
    gt = np.eye(N, dtype=np.float32)[k]
    no_class = rng.random(shape) < .15      # all-zero rows: label values outside the list
    no_class[0, 1, 1, 1] = True
    gt[no_class] = 0.
    logits = (rng.standard_normal(shape + (N,)) * 3.).astype(np.float32)
    z = rng.standard_normal(shape + (N,)) * 2.
    e = np.exp(z - z.max(-1, keepdims=True))
    probs = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    out = dict(gt=gt, logits=logits, probs=probs)
    for name, tv in (('wl2_t5', 5), ('wl2_t3', 3.)):
        out[name] = np.float64(np.asarray(l2i_layers.WeightedL2Loss(target_value=tv)([shim.t(gt), shim.t(logits)])))
    out['ce'] = np.float64(np.asarray(l2i_layers.CrossEntropyLoss(enable_checks=False)([shim.t(gt), shim.t(probs)])))
    np.savez(os.path.join(OUT, 'seg_losses.npz'), **out)
    print({n: (v if np.ndim(v) == 0 else v.shape) for n, v in out.items()})


if __name__ == '__main__':
    main()
