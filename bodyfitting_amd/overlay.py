"""The fit-check overlay of the reference's BodyFitting (smplify/body_fitting.py:34-42 `check_smpl_fitting`, written with --debug for
`use_frames[::render_skip]`, :100-107) on the GPU.

The reference copies the whole view once per vertex and draws one `cv2.circle` at a time.  Here the host does the per-view camera
work in numpy - `w2c = inv(c2w)`, `cv2.Rodrigues(w2c[:3, :3])` (matrix -> vector: SVD orthonormalisation, the `s < 1e-5` branches,
`acos`; returned in the input's depth) and cv2.projectPoints' own vector -> matrix step in double - and one launch of
csrc/overlay_kernels.hip (`bf_overlay_stamp`) projects every vertex of every selected view, in double and in OpenCV's order, rounds to
float32, keeps `0 <= p < W` (and H), truncates with int() and stamps the 5-pixel plus OpenCV's `Circle(radius 1, fill)` draws,
clipped at the edges.  All stamps are (0, 255, 0), so the result does not depend on their order.

`check_smpl_fitting_numpy` / `fit_overlays_numpy` restate the same in numpy; they are the checker of the kernel (tests/), never a
fallback.  None of this has been compared against a cv2 binary: OpenCV's SVD is its own Jacobi SVD, numpy's is
LAPACK's, so R' may differ from cv2's in its last bits.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

GREEN = (0, 255, 0)
CAM_DOUBLES = 21                 # per view: R' [3][3], t [3], K [3][3]


# ---------------------------------------------------------------------------------------------------------------------------------
# the host camera work (both paths)
# ---------------------------------------------------------------------------------------------------------------------------------
def _matmul33(a, b):
    """Matx33d * Matx33d in OpenCV's order: s = 0; s += a(i, k) * b(k, j)"""
    out = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(a[i][k]) * float(b[k][j])
            out[i][j] = s
    return out


def rodrigues_to_vector(R):
    """cv2.Rodrigues of a 3 x 3 rotation (cvRodrigues2's matrix -> vector path) -> rvec [3, 1] in the input's depth (float32 for
    float32, else float64); computed in double"""
    R = np.asarray(R)
    depth = np.float32 if R.dtype == np.float32 else np.float64
    M = R.astype(np.float64).reshape(3, 3)
    if not np.all((M >= -100) & (M < 100)):               # checkRange(R, true, NULL, -100, 100) fails: a zero vector
        return np.zeros((3, 1), depth)
    U, _, Vt = np.linalg.svd(M)
    R = _matmul33(U, Vt)
    rx, ry, rz = R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]
    s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = (R[0][0] + R[1][1] + R[2][2] - 1) * 0.5
    c = 1. if c > 1. else -1. if c < -1. else c
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            rx = ry = rz = 0.0
        else:
            t = (R[0][0] + 1) * 0.5
            rx = math.sqrt(max(t, 0.))
            t = (R[1][1] + 1) * 0.5
            ry = math.sqrt(max(t, 0.)) * (-1. if R[0][1] < 0 else 1.)
            t = (R[2][2] + 1) * 0.5
            rz = math.sqrt(max(t, 0.)) * (-1. if R[0][2] < 0 else 1.)
            if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1][2] > 0) != (ry * rz > 0):
                rz = -rz
            theta /= math.sqrt(rx * rx + ry * ry + rz * rz)
            rx, ry, rz = rx * theta, ry * theta, rz * theta
    else:
        vth = 1 / (2 * s)
        vth *= theta
        rx, ry, rz = rx * vth, ry * vth, rz * vth
    return np.array([[rx], [ry], [rz]], np.float64).astype(depth)


def rodrigues_to_matrix(rvec):
    """cvRodrigues2's vector -> matrix path as cv2.projectPoints runs it (the vector taken to double first) -> float64 [3, 3]"""
    x, y, z = (float(v) for v in np.asarray(rvec, np.float64).reshape(3))
    theta = math.sqrt(x * x + y * y + z * z)
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1. - c
    itheta = 1. / theta if theta else 0.
    x, y, z = x * itheta, y * itheta, z * itheta
    rrt = [[x * x, x * y, x * z], [x * y, y * y, y * z], [x * z, y * z, z * z]]
    r_x = [[0., -z, y], [z, 0., -x], [-y, x, 0.]]
    eye = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]
    # R = c * I + c1 * r r^T + s * [r]_x, element by element in that order
    return np.array([[c * eye[i][j] + c1 * rrt[i][j] + s * r_x[i][j] for j in range(3)] for i in range(3)], np.float64)


def camera(c2w, K):
    """check_smpl_fitting's camera as cv2.projectPoints uses it: (R' float64 [3, 3], t float64 [3], K float64 [3, 3]) from
    w2c = inv(c2w) in the camera's own dtype, rvec = cv2.Rodrigues(w2c[:3, :3]) and back"""
    w2c = np.linalg.inv(np.asarray(c2w))
    rvec = rodrigues_to_vector(w2c[:3, :3])
    return rodrigues_to_matrix(rvec), np.asarray(w2c[:3, 3], np.float64), np.asarray(K, np.float64).reshape(3, 3)


def pack_camera(c2w, K):
    """float64 [21] = R' [9], t [3], K [9]: one view's row of bf_overlay_stamp's cams"""
    R, t, K = camera(c2w, K)
    return np.concatenate([R.reshape(9), t.reshape(3), K.reshape(9)])


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (the checker of the kernel)
# ---------------------------------------------------------------------------------------------------------------------------------
def project_points(verts, R, t, K):
    """cv2.projectPoints(verts.astype(float32), rvec, tvec, K, zeros(5)) with R' = R -> float32 [nv, 2]: double arithmetic in
    cvProjectPoints2Internal's order (only fx, fy, cx, cy of K are read), z = 0 taken as 1 / z = 1"""
    P = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):      # a non-finite vertex is dropped by the bounds test
        x = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
        y = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
        z = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
        z = np.where(z != 0, 1. / np.where(z != 0, z, 1.), 1.)
        x = x * z
        y = y * z
        return np.stack([x * K[0, 0] + K[0, 2], y * K[1, 1] + K[1, 2]], -1).astype(np.float32)


def stamp_numpy(image, points):
    """the loop of check_smpl_fitting on float32 points [nv, 2]: keep 0 <= p < W, 0 <= p < H, int() them and draw
    cv2.circle(r=1, (0, 255, 0), -1) -> a new image"""
    img = np.array(image, copy=True)
    H, W = img.shape[:2]
    p = np.asarray(points, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        keep = (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)
    cx, cy = p[keep, 0].astype(np.int64), p[keep, 1].astype(np.int64)
    for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        x, y = cx + dx, cy + dy
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        img[y[ok], x[ok]] = GREEN
    return img


def check_smpl_fitting_numpy(image, verts, c2w, K):
    """body_fitting.py:34-42 in numpy"""
    R, t, Kd = camera(c2w, K)
    return stamp_numpy(image, project_points(verts, R, t, Kd))


def _views(frames, use_frames):
    use_frames = list(use_frames)
    return [use_frames.index(f) for f in frames]


def fit_overlays_numpy(images, verts, c2ws, Ks, frames, use_frames):
    return [check_smpl_fitting_numpy(images[i], verts, c2ws[i], Ks[i]) for i in _views(frames, use_frames)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------------------
def stamp(images, verts, cams, device=0):
    """bf_overlay_stamp: images (uint8 [H, W, 3] each, one size), verts [nv, 3] (taken to float32), cams float64 [n, 21] (pack_camera)
    -> uint8 [n, H, W, 3]"""
    lib = _lib.load()
    ims = [np.ascontiguousarray(im) for im in images]
    if not ims:
        raise ValueError("overlay.stamp: no views")
    H, W = ims[0].shape[:2]
    for i, im in enumerate(ims):
        if im.dtype != np.uint8 or im.shape != (H, W, 3):
            raise ValueError(f"overlay: view {i} must be uint8 [H, W, 3] of the first view's size ({H}, {W}); got {im.dtype} {im.shape}")
    v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    c = np.ascontiguousarray(np.asarray(cams, np.float64).reshape(len(ims), CAM_DOUBLES))
    out = np.empty((len(ims), H, W, 3), np.uint8)
    ptrs = (C.c_void_p * len(ims))(*[im.ctypes.data for im in ims])
    _lib.check(lib.bf_overlay_stamp(int(device), len(ims), H, W, ptrs, len(v), _lib.fptr(v), c.ctypes.data_as(C.POINTER(C.c_double)),
                                    out.ctypes.data_as(C.POINTER(C.c_uint8))), "bf_overlay_stamp")
    return out


def check_smpl_fitting(image, verts, c2w, K, device=0):
    """body_fitting.py:34-42 check_smpl_fitting(image, verts, c2w, K) on the GPU -> the stamped copy of image"""
    return stamp([image], verts, pack_camera(c2w, K)[None], device)[0]


def fit_overlays(images, verts, c2ws, Ks, frames, use_frames, device=0):
    """body_fitting.py:103-107: the overlay of each view in `frames` (images[i], c2ws[i], Ks[i] at i = use_frames.index(frame)), all in
    one launch per image size -> a list in the order of `frames`"""
    idx = _views(frames, use_frames)
    out = [None] * len(idx)
    groups = {}
    for k, i in enumerate(idx):
        groups.setdefault(np.asarray(images[i]).shape, []).append(k)
    for ks in groups.values():
        cams = np.stack([pack_camera(c2ws[idx[k]], Ks[idx[k]]) for k in ks])
        res = stamp([images[idx[k]] for k in ks], verts, cams, device)
        for j, k in enumerate(ks):
            out[k] = res[j]
    return out
