#!/usr/bin/env python
"""Generate tests/golden/op_set_golden.npz — runs ONLY in the build container (needs torch CPU).

An arbiter for the closed op set that is not the oracle: every row of groups 1 to 9 of tests/op_cases.py is evaluated here with
torch in float64, from the Keras layer documentation.  Nothing of oracle/cnn_oracle.py is used and no padding or pooling
arithmetic is shared with it:

* a stride-1 'same' convolution with odd kernel extents goes through torch's own ``padding='same'``; the cases use no other
  'same' convolution;
* 'same' pooling pads come from ``SAME_PAD``, a table of literals worked out by hand from the TensorFlow documentation's rule
  (pad_along = max((ceil(n / s) - 1) * s + k - n, 0), pad_before = pad_along // 2, the rest after); an entry that is not listed is
  an error;
* a 'same' max pool pads with -inf; a 'same' average pool sums the zero-padded tensor and divides by the same window sums of a
  padded mask of ones (Keras leaves the padding out of the divisor).

The file stores, per case, the float64 output and the float64 tensors of the layers the case names; models and frames are
rebuilt from their seeds at test time.  The archive is written with fixed time stamps, so it regenerates byte for byte.

Usage:  python tests/golden/make_op_set_golden.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import op_cases  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "op_set_golden.npz")

# (extent, pool size, stride) -> (before, after), by hand:
SAME_PAD = {
    # size 3, stride 2: out = ceil(n / 2)
    (5, 3, 2): (1, 1),     # out 3: 4 + 3 - 5 = 2
    (6, 3, 2): (0, 1),     # out 3: 4 + 3 - 6 = 1
    (7, 3, 2): (1, 1),     # out 4: 6 + 3 - 7 = 2
    (8, 3, 2): (0, 1),     # out 4: 6 + 3 - 8 = 1
    (4, 3, 2): (0, 1),     # out 2: 2 + 3 - 4 = 1
    (3, 3, 2): (1, 1),     # out 2: 2 + 3 - 3 = 2
    # size 3, stride 1: out = n, pad_along = 2
    (5, 3, 1): (1, 1), (6, 3, 1): (1, 1), (7, 3, 1): (1, 1), (8, 3, 1): (1, 1), (4, 3, 1): (1, 1), (3, 3, 1): (1, 1),
    # size 2, stride 3 (stride > size): out = ceil(n / 3)
    (5, 2, 3): (0, 0),     # out 2: 3 + 2 - 5 = 0
    (6, 2, 3): (0, 0),     # out 2: 3 + 2 - 6 < 0
    (7, 2, 3): (0, 1),     # out 3: 6 + 2 - 7 = 1
    (8, 2, 3): (0, 0),     # out 3: 6 + 2 - 8 = 0
    (4, 2, 3): (0, 1),     # out 2: 3 + 2 - 4 = 1
    (3, 2, 3): (0, 0),     # out 1: 0 + 2 - 3 < 0
    # size 4, stride 4: out = ceil(n / 4)
    (5, 4, 4): (1, 2),     # out 2: 4 + 4 - 5 = 3
    (6, 4, 4): (1, 1),     # out 2: 4 + 4 - 6 = 2
    (7, 4, 4): (0, 1),     # out 2: 4 + 4 - 7 = 1
    (8, 4, 4): (0, 0),     # out 2: 4 + 4 - 8 = 0
    (4, 4, 4): (0, 0),     # out 1: 0 + 4 - 4 = 0
    (3, 4, 4): (0, 1),     # out 1: 0 + 4 - 3 = 1
    # the anisotropic pool: size (3, 2, 1), stride (2, 1, 1)
    (6, 2, 1): (0, 1),     # out 6: 5 + 2 - 6 = 1
    (4, 2, 1): (0, 1),     # out 4: 3 + 2 - 4 = 1
    (7, 1, 1): (0, 0), (3, 1, 1): (0, 0),
    # size 2, stride 2 on the odd extents of pool_conv_elu_maxpool_same_odd
    (5, 2, 2): (0, 1),     # out 3: 4 + 2 - 5 = 1
    (7, 2, 2): (0, 1),     # out 4: 6 + 2 - 7 = 1
}


def activation(x, name, alpha=None):
    if name in (None, "linear"):
        return x
    if name == "relu":
        return torch.clamp(x, min=0)
    if name == "elu":           # Keras: x if x > 0 else alpha * (exp(x) - 1), for either sign of alpha
        return torch.where(x > 0, x, (1.0 if alpha is None else alpha) * torch.expm1(x))
    if name == "leaky_relu":    # keras.activations.leaky_relu's default slope is 0.2
        return torch.where(x > 0, x, (0.2 if alpha is None else alpha) * x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "softmax":       # over the channels: dim 1 of NCDHW and of [N, F]
        return F.softmax(x, dim=1)
    raise ValueError(name)


def pool(x, c, is_max):
    k, s = tuple(c["pool_size"]), tuple(c["strides"])
    if c["padding"] == "valid":
        return F.max_pool3d(x, k, s) if is_max else F.avg_pool3d(x, k, s)
    pads = [SAME_PAD[(x.shape[2 + a], k[a], s[a])] for a in range(3)]
    tp = (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1])      # torch pads the last axis first
    if is_max:
        return F.max_pool3d(F.pad(x, tp, value=float("-inf")), k, s)
    total = F.avg_pool3d(F.pad(x, tp), k, s, divisor_override=1)
    count = F.avg_pool3d(F.pad(torch.ones((1, 1, *x.shape[2:]), dtype=x.dtype), tp), k, s, divisor_override=1)
    return total / count


def torch_forward(cfg, weights, frames, dt=torch.float64):
    vals = {}
    W = {k: [torch.from_numpy(np.asarray(a)).to(dt) for a in v] for k, v in weights.items()}
    for lc in cfg["config"]["layers"]:
        cn, c, name = lc["class_name"], lc["config"], lc["name"]
        xs = [vals[t[0]] for t in lc["inbound_nodes"][0]] if lc["inbound_nodes"] else []
        w = W.get(name, [])
        if cn == "InputLayer":              # NDHWC -> NCDHW
            y = torch.from_numpy(np.asarray(frames)).to(dt).permute(0, 4, 1, 2, 3).contiguous()
        elif cn == "Conv3D":
            k, s = tuple(c["kernel_size"]), tuple(c["strides"])
            assert s == (1, 1, 1) and tuple(c["dilation_rate"]) == (1, 1, 1), name
            kern = w[0].permute(4, 3, 0, 1, 2).contiguous()     # [kd, kh, kw, Ci, Co] -> [Co, Ci, kd, kh, kw]
            if c["padding"] == "same":
                assert all(kk % 2 == 1 for kk in k), name
                y = F.conv3d(xs[0], kern, w[1] if c["use_bias"] else None, padding="same")
            else:
                y = F.conv3d(xs[0], kern, w[1] if c["use_bias"] else None)
            y = activation(y, c["activation"])
        elif cn == "Dense":
            y = xs[0] @ w[0]
            if c["use_bias"]:
                y = y + w[1]
            y = activation(y, c["activation"])
        elif cn == "BatchNormalization":
            wi = iter(w)
            g = next(wi) if c["scale"] else None
            b = next(wi) if c["center"] else None
            m, v = next(wi), next(wi)
            y = F.batch_norm(xs[0], m, v, g, b, training=False, eps=c["epsilon"])
        elif cn == "ELU":
            y = activation(xs[0], "elu", c["alpha"])
        elif cn == "ReLU":
            assert c["max_value"] is None and c["threshold"] == 0.0
            y = activation(xs[0], "leaky_relu", c["negative_slope"]) if c["negative_slope"] else activation(xs[0], "relu")
        elif cn == "LeakyReLU":
            y = activation(xs[0], "leaky_relu", c["alpha"])
        elif cn == "Softmax":
            y = activation(xs[0], "softmax")
        elif cn == "Activation":
            y = activation(xs[0], c["activation"])
        elif cn in ("MaxPooling3D", "AveragePooling3D"):
            y = pool(xs[0], c, cn == "MaxPooling3D")
        elif cn == "GlobalAveragePooling3D":
            y = xs[0].mean(dim=(2, 3, 4))
        elif cn == "GlobalMaxPooling3D":
            y = xs[0].amax(dim=(2, 3, 4))
        elif cn == "Flatten":               # Keras flattens channels_last: (D, H, W, C) row-major
            y = xs[0].permute(0, 2, 3, 4, 1).reshape(xs[0].shape[0], -1)
        elif cn == "Concatenate":
            y = torch.cat(xs, dim=1)
        elif cn == "Add":
            y = xs[0]
            for o in xs[1:]:
                y = y + o
        else:
            raise ValueError(cn)
        vals[name] = y
    return vals


def to_channels_last(t):
    a = t.numpy()
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)) if a.ndim == 5 else np.ascontiguousarray(a)


def write_npz(path, arrays):
    """np.load reads it like np.savez_compressed's output; the members carry a fixed time stamp, so equal arrays give equal bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    torch.set_num_threads(1)        # one summation order
    out = {}
    for cs in op_cases.CASES:
        if cs.group > 9:
            continue
        cfg, weights, probes = cs.model()
        vals = torch_forward(cfg, weights, cs.frames())
        out[f"{cs.name}__out"] = to_channels_last(vals[cfg["config"]["output_layers"][0][0]])
        for pn in probes:
            out[f"{cs.name}__layer__{pn}"] = to_channels_last(vals[pn])
    write_npz(PATH, out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes,", len(out), "arrays,", sum(a.size for a in out.values()), "values")


if __name__ == "__main__":
    main()
