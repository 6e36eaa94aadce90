"""Conv2DTranspose in float64 and in pairwise fp32, stated through tests/ref64.py: the input zero-stuffed to stride s (x[iy] at row s * iy), then a
stride-1 correlation with the k x k kernel whose window for output row oy starts at stuffed row oy - base, base = k - 1 - p (include/snnhip.h);
"same": p = (k - s) / 2 and s*H x s*W, otherwise p = 0 and s*H + k - s.  The zeros the stuffing adds are exact in both evaluations."""
import numpy as np

import ref64


def geometry(h, w, k, s, same):
    p = (k - s) // 2 if same else 0
    return p, ((s * h, s * w) if same else (s * h + k - s, s * w + k - s))


def _stuffed(x, s):
    n, h, w, c = x.shape
    z = np.zeros((n, s * (h - 1) + 1, s * (w - 1) + 1, c), x.dtype)
    z[:, ::s, ::s] = x
    return z


def deconv_layer(x, w_oihw, bias, s, same, bn=None, act="", alpha=0.0):
    """(float64 reference, pairwise fp32) of deconvolution -> batchnorm -> activation."""
    k = w_oihw.shape[2]
    p, out_hw = geometry(x.shape[1], x.shape[2], k, s, same)
    pads = (k - 1 - p, 0, k - 1 - p, 0)
    y64 = ref64.conv2d_general(_stuffed(np.asarray(x, np.float64), s), w_oihw, bias, 1, pads, "constant", out_hw)
    y32 = ref64.conv2d_pairwise32(_stuffed(np.asarray(x, np.float32), s), w_oihw, bias, 1, pads, "constant", out_hw)
    if bn is not None:
        y64, y32 = ref64.batchnorm(y64, bn), ref64.batchnorm32(y32, bn)
    return ref64.activation(act, y64, alpha), ref64.activation32(act, y32, alpha)
