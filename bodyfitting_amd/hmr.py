"""HMR, the initial estimate of the reference's `BodyFitting.run_hmr` (smplify/body_fitting.py:17-75, models/hmr.py), on the GPU.

The network runs in `libbodyfit.so` (csrc/hmr_kernels.hip, hmr_api.hip) in fp32; this module reads the weights without torch,
folds each BatchNorm into its convolution, packs the layers in the order the C side walks them, and finishes on the host what
touches 24 joints per image: rot6d_to_rotmat, the caller's root rotation and convert_hom_to_angle (utils/geometry.py:100-114,331-493),
in numpy float32 and in the reference's operation order.

Weights come from `assets.get_hmr()`: the arrays registered with `assets.register_hmr(...)`, else the reference's own files
`data/model_checkpoint.pt` (config.HMR_CHECKPOINT, a `torch.save` file, zip or legacy format) and `data/smpl_mean_params.npz`
(config.SMPL_MEAN_PARAMS).

The BatchNorm fold (eval(): running statistics, eps 1e-5) is done in float64 and rounded once to float32.  It changes the rounding
order against the reference (conv, then (x - mean) / sqrt(var + eps) * gamma + beta, each in fp32); the GPU tests' error band
 is set by the reference's own fp32 error and covers it.
"""
from __future__ import annotations

import collections
import io
import os
import pickle
import struct
import zipfile

import numpy as np

from . import _lib

RES = 224
IMG_NORM_MEAN = (0.485, 0.456, 0.406)          # constants.py:4-5
IMG_NORM_STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5
BLOCKS, PLANES, STRIDES = (3, 4, 6, 3), (64, 128, 256, 512), (1, 2, 2, 2)
NPOSE, NSTATE, NFEAT = 144, 157, 2048

# ---------------------------------------------------------------------------------------------------------------------------------
# torch.save files without torch
# ---------------------------------------------------------------------------------------------------------------------------------
_STORAGE_DTYPES = {
    "FloatStorage": np.float32, "DoubleStorage": np.float64, "HalfStorage": np.float16, "BFloat16Storage": None,
    "LongStorage": np.int64, "IntStorage": np.int32, "ShortStorage": np.int16, "CharStorage": np.int8,
    "ByteStorage": np.uint8, "BoolStorage": np.bool_,
}
_LEGACY_MAGIC = 0x1950a86a20f9469cfc6c


class _StorageType:
    def __init__(self, name):
        dtype = _STORAGE_DTYPES[name]
        if dtype is None:
            raise pickle.UnpicklingError(f"unsupported storage type torch.{name}")
        self.dtype = np.dtype(dtype)


class _Storage:
    def __init__(self, stype, key):
        self.dtype, self.key, self.array = stype.dtype, key, None


class _Tensor:
    """a tensor whose storage may not have been read yet (legacy files keep the bytes after the pickle)"""
    def __init__(self, storage, offset, size, stride):
        self.storage, self.offset, self.size, self.stride = storage, int(offset), tuple(size), tuple(stride)

    def numpy(self):
        a = self.storage.array
        if a is None:
            raise pickle.UnpicklingError(f"storage {self.storage.key!r} has no data")
        isz = a.dtype.itemsize
        if self.size and max((s - 1) * st for s, st in zip(self.size, self.stride)) + self.offset >= max(a.size, 1) and 0 not in self.size:
            raise pickle.UnpicklingError("tensor reaches beyond its storage")
        return np.lib.stride_tricks.as_strided(a[self.offset:], self.size, [st * isz for st in self.stride]).copy()


def _rebuild_tensor(storage, offset, size, stride, *rest):
    return _Tensor(storage, offset, size, stride)


def _rebuild_parameter(data, requires_grad, backward_hooks, *rest):
    return data


class _RestrictedUnpickler(pickle.Unpickler):
    """resolves the tensor-rebuild and storage globals of torch.save and collections.OrderedDict - nothing else is looked up,
    let alone called"""

    def __init__(self, f, storages):
        super().__init__(f)
        self._storages = storages

    def find_class(self, module, name):
        if module == "collections" and name == "OrderedDict":
            return collections.OrderedDict
        if module == "torch._utils" and name in ("_rebuild_tensor", "_rebuild_tensor_v2"):
            return _rebuild_tensor
        if module == "torch._utils" and name == "_rebuild_parameter":
            return _rebuild_parameter
        if module == "torch" and name in _STORAGE_DTYPES:
            return _StorageType(name)
        raise pickle.UnpicklingError(f"refusing to load the global {module}.{name} from a checkpoint")

    def persistent_load(self, pid):
        if not (isinstance(pid, tuple) and len(pid) >= 5 and pid[0] == "storage" and isinstance(pid[1], _StorageType)):
            raise pickle.UnpicklingError(f"unsupported persistent id {pid!r}")
        key = str(pid[2])
        if key not in self._storages:
            self._storages[key] = _Storage(pid[1], key)
        if len(pid) > 5 and pid[5] is not None:
            raise pickle.UnpicklingError("storage views of the legacy format are not supported")
        return self._storages[key]


def _resolve(obj):
    if isinstance(obj, _Tensor):
        return obj.numpy()
    if isinstance(obj, collections.OrderedDict):
        return collections.OrderedDict((k, _resolve(v)) for k, v in obj.items())
    if isinstance(obj, dict):
        return {k: _resolve(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_resolve(v) for v in obj]
    if isinstance(obj, tuple):
        return tuple(_resolve(v) for v in obj)
    return obj


def load_checkpoint(path):
    """`torch.load(path)` for tensors and plain containers, without torch: tensors come back as numpy arrays.  Reads the zip
    format and the legacy pickle-stream format of torch.save."""
    storages = {}
    if zipfile.is_zipfile(path):
        with zipfile.ZipFile(path) as z:
            pkl = [n for n in z.namelist() if n.endswith("/data.pkl") or n == "data.pkl"]
            if len(pkl) != 1:
                raise ValueError(f"{path}: not a torch.save archive (no single data.pkl)")
            root = pkl[0][:-len("data.pkl")]
            obj = _RestrictedUnpickler(io.BytesIO(z.read(pkl[0])), storages).load()
            for key, st in storages.items():
                st.array = np.frombuffer(z.read(f"{root}data/{key}"), dtype=st.dtype.newbyteorder("<"))
        return _resolve(obj)
    with open(path, "rb") as f:
        plain = _RestrictedUnpickler(f, {})
        if plain.load() != _LEGACY_MAGIC:
            raise ValueError(f"{path}: not a torch.save file (bad magic number)")
        if plain.load() != 1001:
            raise ValueError(f"{path}: unsupported torch.save protocol")
        info = plain.load()
        if not info.get("little_endian", True):
            raise ValueError(f"{path}: big-endian checkpoints are not supported")
        obj = _RestrictedUnpickler(f, storages).load()
        keys = _RestrictedUnpickler(f, {}).load()
        for key in keys:
            st = storages[str(key)]
            n, = struct.unpack("<q", f.read(8))
            raw = f.read(n * st.dtype.itemsize)
            if len(raw) != n * st.dtype.itemsize:
                raise ValueError(f"{path}: truncated storage {key}")
            st.array = np.frombuffer(raw, dtype=st.dtype.newbyteorder("<"))
    return _resolve(obj)


# ---------------------------------------------------------------------------------------------------------------------------------
# the network's parameters
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_layers():
    """(conv key prefix, bn key prefix, cin, cout, k, stride, pad) in the order hmr_api.hip walks them"""
    out = [("conv1", "bn1", 3, 64, 7, 2, 3)]
    inplanes = 64
    for li, (nb, p, s0) in enumerate(zip(BLOCKS, PLANES, STRIDES)):
        for b in range(nb):
            pre, s = f"layer{li + 1}.{b}.", s0 if b == 0 else 1
            out.append((pre + "conv1", pre + "bn1", inplanes, p, 1, 1, 0))
            out.append((pre + "conv2", pre + "bn2", p, p, 3, s, 1))
            out.append((pre + "conv3", pre + "bn3", p, 4 * p, 1, 1, 0))
            if b == 0:
                out.append((pre + "downsample.0", pre + "downsample.1", inplanes, 4 * p, 1, s, 0))
            inplanes = 4 * p
    return out


FC_LAYERS = (("fc1", NFEAT + NSTATE, 1024), ("fc2", 1024, 1024), ("decpose", 1024, NPOSE), ("decshape", 1024, 10), ("deccam", 1024, 3))
BUFFERS = (("init_pose", NPOSE), ("init_shape", 10), ("init_cam", 3))


def expected_shapes():
    """every entry of HMR(Bottleneck, [3, 4, 6, 3]).state_dict() -> shape"""
    shapes = collections.OrderedDict()
    for conv, bn, cin, cout, k, _, _ in conv_layers():
        shapes[conv + ".weight"] = (cout, cin, k, k)
        for name in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{bn}.{name}"] = (cout,)
        shapes[bn + ".num_batches_tracked"] = ()
    for name, fin, fout in FC_LAYERS:
        shapes[name + ".weight"] = (fout, fin)
        shapes[name + ".bias"] = (fout,)
    for name, n in BUFFERS:
        shapes[name] = (1, n)
    return shapes


def match_state(checkpoint_model, filename, mean_params=None):
    """`HMR_forward`'s load_state_dict (smplify/body_fitting.py:21-27) on a checkpoint's 'model' dict -> the parameters by key.

    `model_checkpoint.pt`: strict=False, unexpected keys are ignored.  Any other name: `module.` prefixes stripped, strict=True.
    Unlike the reference, a missing convolution, BatchNorm or linear entry is a ValueError naming it (torch would keep the
    random initialisation).  init_pose / init_shape / init_cam come from the checkpoint when it has them, else from mean_params
    (the npz the constructor reads first)."""
    shapes = expected_shapes()
    strict = os.path.basename(str(filename)) != "model_checkpoint.pt"
    sd = dict(checkpoint_model)
    if strict:
        sd = {k.replace("module.", ""): v for k, v in sd.items()}
        unexpected = sorted(k for k in sd if k not in shapes)
        if unexpected:
            raise ValueError(f"{filename}: unexpected key(s) in the HMR state dict (strict load): {', '.join(unexpected[:5])}")
    out = {}
    for key, shape in shapes.items():
        if key in sd:
            v = np.asarray(sd[key])
            if tuple(v.shape) != shape:
                raise ValueError(f"{filename}: {key} has shape {tuple(v.shape)}, HMR needs {shape}")
            out[key] = v
        elif key.endswith("num_batches_tracked") and not strict:
            continue
        elif key in dict(BUFFERS) and mean_params is not None and not strict:
            out[key] = np.asarray(mean_params[{"init_pose": "pose", "init_shape": "shape", "init_cam": "cam"}[key]],
                                  np.float32).reshape(shape)
        else:
            raise ValueError(f"{filename}: the HMR weights have no {key!r}")
    return out


def fold_and_pack(state):
    """-> (packed float32 weights in hmr_api.hip's order, mean state float32[157]).  Each BatchNorm is folded into its convolution
    in float64: w' = w * g / sqrt(var + eps), b' = beta - mean * g / sqrt(var + eps); rounded to float32 once."""
    parts = []
    for conv, bn, cin, cout, k, _, _ in conv_layers():
        w, b = fold_conv_bn(state, conv, bn)
        parts += [w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout), b]           # [K = (ky, kx, ci)][Cout]
    for name in ("fc1", "fc2"):
        parts += [np.asarray(state[name + ".weight"], np.float64).T, np.asarray(state[name + ".bias"], np.float64)]
    dec = ("decpose", "decshape", "deccam")
    parts += [np.concatenate([np.asarray(state[d + ".weight"], np.float64) for d in dec], 0).T,
              np.concatenate([np.asarray(state[d + ".bias"], np.float64) for d in dec])]
    packed = np.concatenate([p.astype(np.float32).ravel() for p in parts])
    mean = np.concatenate([np.asarray(state[n], np.float32).ravel() for n, _ in BUFFERS])
    return packed, mean


def fold_conv_bn(state, conv, bn):
    """float64 (w' [cout, cin, k, k], b' [cout]) of conv followed by eval-mode BatchNorm"""
    w = np.asarray(state[conv + ".weight"], np.float64)
    scale = np.asarray(state[bn + ".weight"], np.float64) / np.sqrt(np.asarray(state[bn + ".running_var"], np.float64) + BN_EPS)
    b = np.asarray(state[bn + ".bias"], np.float64) - np.asarray(state[bn + ".running_mean"], np.float64) * scale
    return w * scale[:, None, None, None], b


def weights_digest(state):
    import hashlib
    h = hashlib.sha256()
    for key in expected_shapes():
        if key in state and not key.endswith("num_batches_tracked"):
            h.update(key.encode())
            h.update(np.ascontiguousarray(state[key], np.float32).tobytes())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------------------------
# the image pipeline and the post-processing (host restatements; the kernel's is csrc/hmr_kernels.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_image(image):
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"HMR takes uint8 RGB images [H, W, 3]; got {a.dtype} {a.shape}")
    return a


def _axis(n_src, clamp_weight):
    scale = n_src / RES
    f = ((np.arange(RES) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_weight:
        lo, hi = s < 0, s >= n_src - 1
        f[lo], s[lo] = 0, 0
        f[hi], s[hi] = 0, n_src - 1
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), a0, a1


def resize_224(image):
    """cv2.resize(image, (224, 224)) as run_hmr calls it - INTER_LINEAR on uint8 (see csrc/hmr_kernels.hip), integer arithmetic"""
    img = check_image(image).astype(np.int64)
    H, W = img.shape[:2]
    x0, x1, a0, a1 = _axis(W, True)
    y0, y1, b0, b1 = _axis(H, False)
    edge = x0 == W - 1
    h = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
    h[:, edge] = img[:, x0[edge]] * 2048
    v = (((b0[:, None, None] * (h[y0] >> 4)) >> 16) + ((b1[:, None, None] * (h[y1] >> 4)) >> 16) + 2) >> 2
    return v.astype(np.uint8)


def normalize(resized):
    """/255 and transforms.Normalize(IMG_NORM_MEAN, IMG_NORM_STD) in float32, NHWC"""
    x = np.asarray(resized).astype(np.float32) / np.float32(255)
    return (x - np.asarray(IMG_NORM_MEAN, np.float32)) / np.asarray(IMG_NORM_STD, np.float32)


def rot6d_to_rotmat(x):
    """utils/geometry.py:100-114 in float32: [B, 6] (or [n, 144]) -> [B, 3, 3] (columns b1, b2, b3)"""
    x = np.asarray(x, np.float32).reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]

    def _normalize(v):
        return v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), np.float32(1e-12))
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum(1, keepdims=True) * b1)
    b3 = np.cross(b1, b2).astype(np.float32)
    return np.stack((b1, b2, b3), axis=-1)


def rotation_matrix_to_quaternion(R, eps=1e-6):
    """torchgeometry's rotation_matrix_to_quaternion (utils/geometry.py:401-475) in float32 on R[N, 3, 3]"""
    R = np.asarray(R, np.float32)
    t = np.transpose(R, (0, 2, 1))             # rmat_t[:, i, j] = R[:, j, i]
    one = np.float32(1)
    mask_d2 = t[:, 2, 2] < eps
    mask_d0_d1 = t[:, 0, 0] > t[:, 1, 1]
    mask_d0_nd1 = t[:, 0, 0] < -t[:, 1, 1]
    t0 = one + t[:, 0, 0] - t[:, 1, 1] - t[:, 2, 2]
    q0 = np.stack([t[:, 1, 2] - t[:, 2, 1], t0, t[:, 0, 1] + t[:, 1, 0], t[:, 2, 0] + t[:, 0, 2]], -1)
    t1 = one - t[:, 0, 0] + t[:, 1, 1] - t[:, 2, 2]
    q1 = np.stack([t[:, 2, 0] - t[:, 0, 2], t[:, 0, 1] + t[:, 1, 0], t1, t[:, 1, 2] + t[:, 2, 1]], -1)
    t2 = one - t[:, 0, 0] - t[:, 1, 1] + t[:, 2, 2]
    q2 = np.stack([t[:, 0, 1] - t[:, 1, 0], t[:, 2, 0] + t[:, 0, 2], t[:, 1, 2] + t[:, 2, 1], t2], -1)
    t3 = one + t[:, 0, 0] + t[:, 1, 1] + t[:, 2, 2]
    q3 = np.stack([t3, t[:, 1, 2] - t[:, 2, 1], t[:, 2, 0] - t[:, 0, 2], t[:, 0, 1] - t[:, 1, 0]], -1)
    c0 = (mask_d2 & mask_d0_d1).astype(np.float32)[:, None]
    c1 = (mask_d2 & ~mask_d0_d1).astype(np.float32)[:, None]
    c2 = (~mask_d2 & mask_d0_nd1).astype(np.float32)[:, None]
    c3 = (~mask_d2 & ~mask_d0_nd1).astype(np.float32)[:, None]
    q = q0 * c0 + q1 * c1 + q2 * c2 + q3 * c3
    with np.errstate(invalid="ignore"):
        q = q / np.sqrt(t0[:, None] * c0 + t1[:, None] * c1 + t2[:, None] * c2 + t3[:, None] * c3)
    return (q * np.float32(0.5)).astype(np.float32)


def quaternion_to_angle_axis(q):
    """torchgeometry's quaternion_to_angle_axis (utils/geometry.py:350-398) in float32"""
    q = np.asarray(q, np.float32)
    q1, q2, q3 = q[..., 1], q[..., 2], q[..., 3]
    sin_sq = q1 * q1 + q2 * q2 + q3 * q3
    sin_t = np.sqrt(sin_sq)
    cos_t = q[..., 0]
    two_theta = np.float32(2) * np.where(cos_t < 0, np.arctan2(-sin_t, -cos_t), np.arctan2(sin_t, cos_t)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(sin_sq > 0, two_theta / sin_t, np.float32(2)).astype(np.float32)
    return np.stack([q1 * k, q2 * k, q3 * k], -1).astype(np.float32)


def convert_hom_to_angle(rotmat):
    """utils/geometry.py:478-487: rotmat[n, 24, 3, 3] -> pose[n, 72], NaN -> 0"""
    rotmat = np.asarray(rotmat, np.float32)
    n = rotmat.shape[0]
    pose = quaternion_to_angle_axis(rotation_matrix_to_quaternion(rotmat.reshape(-1, 3, 3))).reshape(n, -1)
    pose[np.isnan(pose)] = 0.0
    return pose


def apply_root(rotmat, c2ws):
    """run_hmr's `pred_rotmat[0, 0] = c2w[:3, :3] @ smpl_rot` for every image (float32 matmul)"""
    rotmat = np.array(rotmat, np.float32)
    if c2ws is not None:
        c2ws = np.asarray(c2ws, np.float32).reshape(-1, 4, 4)
        if c2ws.shape[0] != rotmat.shape[0]:
            raise ValueError(f"{rotmat.shape[0]} images but {c2ws.shape[0]} c2w matrices")
        rotmat[:, 0] = np.matmul(c2ws[:, :3, :3], rotmat[:, 0])
    return rotmat


# ---------------------------------------------------------------------------------------------------------------------------------
# the device network
# ---------------------------------------------------------------------------------------------------------------------------------
class HMR:
    """HMR(weights=None, mean_params=None, device=0, max_batch=32).  `weights`: a state dict (the checkpoint's 'model' entry,
    already key-matched) or None for `assets.get_hmr()`; `mean_params`: a dict with pose / shape / cam when the state dict
    lacks init_pose / init_shape / init_cam."""

    def __init__(self, weights=None, mean_params=None, device=0, max_batch=32):
        import ctypes as C
        if weights is None:
            from . import assets
            packed, mean = assets.get_hmr()
        else:
            packed, mean = fold_and_pack(match_state(weights, "model_checkpoint.pt", mean_params))
        self._lib = _lib.load()
        n = int(self._lib.bf_hmr_n_weights())
        if packed.size != n:
            raise ValueError(f"{packed.size} packed HMR weights, the network has {n}")
        self.max_batch, self.device = int(max_batch), int(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_hmr_create(self.device, _lib.fptr(np.ascontiguousarray(packed)), n, _lib.fptr(np.ascontiguousarray(mean)),
                                           self.max_batch, C.byref(self._h)), "bf_hmr_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bf_hmr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _groups(self, images):
        """images: uint8 [n, H, W, 3] or a list of [H, W, 3] -> chunks (indices, [k, H, W, 3]) of one size and <= max_batch"""
        if isinstance(images, np.ndarray) and images.ndim == 4:
            images = list(images)
        imgs = [check_image(im) for im in images]
        by_size = collections.OrderedDict()
        for i, im in enumerate(imgs):
            by_size.setdefault(im.shape, []).append(i)
        for idx in by_size.values():
            for s in range(0, len(idx), self.max_batch):
                part = idx[s:s + self.max_batch]
                yield part, np.ascontiguousarray(np.stack([imgs[i] for i in part]))

    def _u8(self, a):
        import ctypes as C
        return a.ctypes.data_as(C.POINTER(C.c_uint8))

    def preprocess(self, images):
        """-> (resized uint8 [n, 224, 224, 3], normalised float32 [n, 224, 224, 3]) from the device"""
        chunks = list(self._groups(images))
        n = sum(len(p) for p, _ in chunks)
        res, nrm = np.zeros((n, RES, RES, 3), np.uint8), np.zeros((n, RES, RES, 3), np.float32)
        for part, a in chunks:
            r, f = np.zeros((len(part), RES, RES, 3), np.uint8), np.zeros((len(part), RES, RES, 3), np.float32)
            _lib.check(self._lib.bf_hmr_preprocess(self._h, len(part), a.shape[1], a.shape[2], self._u8(a), self._u8(r), _lib.fptr(f)),
                       "bf_hmr_preprocess")
            res[part], nrm[part] = r, f
        return res, nrm

    def features(self, images):
        """the pooled layer-4 features xf[n, 2048]"""
        chunks = list(self._groups(images))
        xf = np.zeros((sum(len(p) for p, _ in chunks), NFEAT), np.float32)
        for part, a in chunks:
            out = np.zeros((len(part), NFEAT), np.float32)
            _lib.check(self._lib.bf_hmr_features(self._h, len(part), a.shape[1], a.shape[2], self._u8(a), _lib.fptr(out)), "bf_hmr_features")
            xf[part] = out
        return xf

    def regress(self, images):
        """the regressor's final state: (pose6d [n, 144], betas [n, 10], cam [n, 3])"""
        chunks = list(self._groups(images))
        n = sum(len(p) for p, _ in chunks)
        pose6d, betas, cam = np.zeros((n, NPOSE), np.float32), np.zeros((n, 10), np.float32), np.zeros((n, 3), np.float32)
        for part, a in chunks:
            p6, b, c = np.zeros((len(part), NPOSE), np.float32), np.zeros((len(part), 10), np.float32), np.zeros((len(part), 3), np.float32)
            _lib.check(self._lib.bf_hmr_predict(self._h, len(part), a.shape[1], a.shape[2], self._u8(a), _lib.fptr(p6), _lib.fptr(b),
                                                _lib.fptr(c)), "bf_hmr_predict")
            pose6d[part], betas[part], cam[part] = p6, b, c
        return pose6d, betas, cam

    def forward(self, images):
        """HMR.forward's outputs (pred_rotmat [n, 24, 3, 3], pred_betas [n, 10], pred_camera [n, 3])"""
        pose6d, betas, cam = self.regress(images)
        return rot6d_to_rotmat(pose6d).reshape(-1, 24, 3, 3), betas, cam

    def predict(self, images, c2ws=None):
        """run_hmr per image: (pred_betas [n, 10], pred_poses [n, 72]) with each root rotation taken to world by its c2w"""
        rotmat, betas, _ = self.forward(images)
        return betas, convert_hom_to_angle(apply_root(rotmat, c2ws))
