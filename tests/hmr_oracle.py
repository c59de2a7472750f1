"""A torch-CPU restatement of the reference's HMR (models/hmr.py: ResNet-50 v1.5 in eval() + the iterative regressor) on a state
dict of numpy arrays, with BatchNorm as the reference runs it (unfolded) or folded as bodyfitting_amd.hmr packs it.  The checker,
never the product: the GPU tests compare the HIP network with tests/golden/hmr_*.npz, which tools/gen_hmr_golden.py writes with the
reference's own module, and this file reproduces that golden on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from bodyfitting_amd import hmr as H


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _conv_bn(state, x, conv, bn, stride, pad, dtype, folded):
    if folded:
        w, b = H.fold_conv_bn(state, conv, bn)
        return F.conv2d(x, _t(w, dtype), _t(b, dtype), stride=stride, padding=pad)
    y = F.conv2d(x, _t(state[conv + ".weight"], dtype), None, stride=stride, padding=pad)
    return F.batch_norm(y, _t(state[bn + ".running_mean"], dtype), _t(state[bn + ".running_var"], dtype),
                        _t(state[bn + ".weight"], dtype), _t(state[bn + ".bias"], dtype), False, 0.0, H.BN_EPS)


def backbone(state, x, dtype=torch.float64, folded=False, return_layer4=False):
    """x [n, 3, 224, 224] (NCHW, normalised) -> xf [n, 2048]"""
    layers = H.conv_layers()
    x = x.to(dtype)
    conv, bn, *_, s, p = layers[0]
    x = F.max_pool2d(F.relu(_conv_bn(state, x, conv, bn, s, p, dtype, folded)), 3, 2, 1)
    i = 1
    for nb in H.BLOCKS:
        for b in range(nb):
            c1, c2, c3 = layers[i:i + 3]
            out = F.relu(_conv_bn(state, x, c1[0], c1[1], c1[5], c1[6], dtype, folded))
            out = F.relu(_conv_bn(state, out, c2[0], c2[1], c2[5], c2[6], dtype, folded))
            out = _conv_bn(state, out, c3[0], c3[1], c3[5], c3[6], dtype, folded)
            if b == 0:
                ds = layers[i + 3]
                res = _conv_bn(state, x, ds[0], ds[1], ds[5], ds[6], dtype, folded)
                i += 4
            else:
                res = x
                i += 3
            x = F.relu(out + res)
    xf = F.avg_pool2d(x, 7, 1).reshape(x.shape[0], -1)
    return (xf, x) if return_layer4 else xf


def regressor(state, xf, dtype=torch.float64, n_iter=3):
    """-> (pose6d [n, 144], betas [n, 10], cam [n, 3])"""
    n = xf.shape[0]
    pose, shape, cam = (_t(state[k], dtype).reshape(1, -1).expand(n, -1) for k in ("init_pose", "init_shape", "init_cam"))

    def lin(name, v):
        return F.linear(v, _t(state[name + ".weight"], dtype), _t(state[name + ".bias"], dtype))
    for _ in range(n_iter):
        xc = lin("fc2", lin("fc1", torch.cat([xf.to(dtype), pose, shape, cam], 1)))
        pose, shape, cam = lin("decpose", xc) + pose, lin("decshape", xc) + shape, lin("deccam", xc) + cam
    return pose, shape, cam


def network_input(images):
    """the run_hmr pipeline with bodyfitting_amd.hmr's resize restatement -> (resized uint8 [n, 224, 224, 3], x [n, 3, 224, 224] fp32)"""
    resized = np.stack([H.resize_224(im) for im in images])
    x = torch.from_numpy(resized).float() / 255.
    x = (x - torch.tensor(H.IMG_NORM_MEAN)) / torch.tensor(H.IMG_NORM_STD)
    return resized, x.permute(0, 3, 1, 2).contiguous()


def rot6d_to_rotmat(x):
    x = x.reshape(-1, 3, 2)
    b1 = F.normalize(x[:, :, 0])
    b2 = F.normalize(x[:, :, 1] - torch.einsum("bi,bi->b", b1, x[:, :, 1]).unsqueeze(-1) * b1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)
