"""`smplify.loss` of the reference (smplify/loss.py) on the HIP path: `multiview_keypoint_loss` - the reprojection term over the
views, MaxMixturePrior's merged likelihood, the angle prior and the shape prior - as ONE kernel launch (bf_keypoint_loss) and,
for torch tensors, its vector-Jacobian product behind a torch.autograd.Function.  This is the second half of a user's own
optimisation loop (smplify.py:177-213); the first half is the body model (smpl.py, smplx.py).

torch tensors in -> (total, losses) with `total` a float32 scalar tensor on model_joints' device, differentiable (once) with respect
to model_joints, poses and betas; numpy in -> floats out.  torch is imported only when tensors arrive.  float32 tensors on the
prior's GPU go into the kernel where they lie, on torch's current stream (bf_keypoint_loss_dev: the device route of
_autograd.py); the packed views are sent to that GPU once per distinct set of cameras and keypoints and remembered (four sets),
and `losses`' four host values are the one read-back of a call.  Everything else goes through host memory.

`perspective_projection`, `gmof`, `angle_prior` and `reprojection_loss` are the reference's small functions, in torch or numpy as
their arguments are.

The scan term and the SMPL+D stage's losses of that loop (smplify.py:205-206,236-245) are here too, each one HIP call that returns
the gradient for cotangent 1 with the value: `point_cloud_loss_mesh_grid` (bf_scan_point_loss: the search, then one Frobenius norm;
the gradient goes to `points`), `normal_loss_mesh_grid` (bf_normal_loss, to `point_norm`) and `normal_laplacian_smoothness`
(bf_normal_laplacian, to `norms`); `compute_normal_torch` is in normals.py.  torch tensors in -> a 0-dim float32 tensor on the
inputs' device, differentiable once; numpy in -> a float.  The two scan losses of one iteration query the same points: the searcher
keeps its last query's answer, so the second one does not search again.  float32 tensors on the scan's / the topology's GPU take
the device route (bf_scan_point_loss_dev, bf_normal_loss_dev, bf_normal_laplacian_dev): addresses in, the loss a tensor that never
leaves the GPU, the closest faces' normals gathered in the kernel, the backward a scaling launch that reads the cotangent where it
lies; the searcher's memo is then the points TENSOR, held, by identity and version (mesh_grid_searcher.memo_hit).
They take this project's MeshGridSearcher, arrays and
tensors; anything else raises NotImplementedError (SMPLify's fused stage is the other path), every other refusal is a ValueError.

The silhouette term of that loop (smplify.py:144,198) is here as well: `extract_countours` follows the masks' external borders on
the GPU and keeps masks and contours there (a `native.Silhouette`, remembered per masks object and GPU), and `multview_mask_loss`
evaluates the loss on the vertices the caller holds as ONE bf_silhouette_loss call - three launches - whose gradient goes to
`smpl_verts`.  On the device route (float32 / uint8 / bool masks and float32 vertices on that GPU) nothing crosses to the host:
the masks go in by address (bf_silhouette_create_dev), the contours come back as GPU tensors, the cameras are stacked on the GPU
once per distinct set (four sets remembered) and the loss is bf_silhouette_loss_dev on torch's current stream.  The chamfer loss (called nowhere in the reference) runs nowhere: its stand-alone version raises NotImplementedError.
"""
from __future__ import annotations

import numpy as np

from . import _autograd
from . import _memo
from . import normals as _normals
from .keypoints import FACE_MAPPING, pack_keypoints_smplx          # noqa: F401  (FACE_MAPPING: a name of loss.py, re-exported)
from . import prior as _prior

SKELETON_LENGTH = 25          # loss.py:17-20
HANDS_LENGTH = 42
FACE_LENGTH = 68
LOSS_KEYS = ("reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")
_ANGLE_IDX, _ANGLE_SIGN = [55 - 3, 58 - 3, 12 - 3, 15 - 3], [1.0, -1.0, -1.0, -1.0]


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "requires_grad")


def _host(a, dtype=np.float32):
    return np.asarray(a.detach().cpu().numpy() if _is_tensor(a) else a, dtype)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference's small functions (loss.py:22-61,132-136)
# ----------------------------------------------------------------------------------------------------------------------------

def perspective_projection(points, rotation, translation, K):
    """points[bs,N,3], rotation[bs,3,3], translation[bs,3], K[3,3] -> [bs,N,2] (loss.py:22-43: no epsilon on the depth)"""
    if _is_tensor(points):
        import torch
        K = torch.as_tensor(np.asarray(K), dtype=torch.float32, device=points.device) if isinstance(K, np.ndarray) else K
        cam = torch.einsum("bij,bkj->bki", rotation, points) + translation.unsqueeze(1)
        pix = torch.einsum("ij,bkj->bki", K, cam)
    else:
        points, rotation, translation, K = (np.asarray(a) for a in (points, rotation, translation, K))
        cam = np.einsum("bij,bkj->bki", rotation, points) + translation[:, None]
        pix = np.einsum("ij,bkj->bki", K, cam)
    return (pix / pix[:, :, -1:])[:, :, :-1]


def gmof(x, sigma):
    """Geman-McClure error function (loss.py:45-51)"""
    x_squared, sigma_squared = x ** 2, sigma ** 2
    return (sigma_squared * x_squared) / (sigma_squared + x_squared)


def angle_prior(pose):
    """exp(theta * sign) ** 2 on the knees' and elbows' bending dofs (loss.py:54-61), pose[B, >= 56] -> [B, 4]"""
    if _is_tensor(pose):
        import torch
        return torch.exp(pose[:, _ANGLE_IDX] * torch.tensor(_ANGLE_SIGN, device=pose.device, dtype=pose.dtype)) ** 2
    pose = np.asarray(pose)
    return np.exp(pose[:, _ANGLE_IDX] * np.asarray(_ANGLE_SIGN, pose.dtype)) ** 2


def reprojection_loss(cord, cord_gt, conf, scale_coeff, sigma):
    """loss.py:132-136"""
    err = gmof((cord_gt - cord) / scale_coeff, sigma)
    return ((conf ** 2) * err.sum(-1)).sum(-1)


def _fused_only(name):
    def stub(*args, **kwargs):
        raise NotImplementedError(f"smplify.loss.{name}: SMPLify runs this loss fused inside its fit kernels "
                                  "(bodyfitting_amd.smplify); the stand-alone differentiable version is a follow-up")
    stub.__name__ = name
    return stub


point_cloud_loss_chamfer_naive = _fused_only("point_cloud_loss_chamfer_naive")


# ----------------------------------------------------------------------------------------------------------------------------
# the scan term and the SMPL+D stage's losses (loss.py:233-242,260-288)
# ----------------------------------------------------------------------------------------------------------------------------

def _scalar_loss(who, x, call, plus_zero=False, device=None, device_call=None):
    """`call(array, want_grad)` -> (value, gradient for cotangent 1 or None): ONE native call per evaluation - the gradient comes
    back with the value when `x` asks for one, and the backward only scales it.  -> a 0-dim tensor on x's device, or a float.
    plus_zero: the scaled gradient's zeros are +0 whatever the cotangent's sign (0 * -2.5 is -0).
    device, device_call: the GPU a device route is offered on (None: none) and `device_call(tensor, want_grad, stream)` -> (value
    tensor [1], gradient tensor or None) on it (_autograd.ScalarLossRoute); taken when _autograd.route_for says so for `x`."""
    if not _is_tensor(x):
        return float(call(x, False)[0])
    import torch
    kept = []
    want_grad = bool(x.requires_grad and torch.is_grad_enabled())          # (read here: grad mode is off inside a Function's forward)

    def forward(a):
        value, grad = call(a, want_grad)
        kept.append(grad)
        return (np.asarray(value).reshape(1),)

    def vjp(arrays, cotangents):
        if kept[0] is None:
            raise RuntimeError(f"{who}: no gradient was computed with the forward")
        scaled = kept[0] * np.asarray(cotangents[0]).reshape(-1)[0]
        return (scaled + 0.0 if plus_zero else scaled,)

    route = None if device_call is None else _autograd.ScalarLossRoute(who, device, device_call, want_grad, plus_zero)
    return _autograd.apply(forward, vjp, (x,), device_route=route)[0].reshape(())


_takes_device_route = _autograd.takes_device_route


def _new(like, shape, dtype=None):
    import torch
    return torch.empty(shape, dtype=dtype or torch.float32, device=like.device)


def _value_and_grad(x, want_grad, n_values=1):          # (what a `device_call` of _scalar_loss fills, on x's GPU)
    return _new(x, n_values), (_new(x, x.shape) if want_grad else None)


def _scan_of(who, mesh_grid_searcher):
    from .mesh_grid_searcher import MeshGridSearcher
    if not isinstance(mesh_grid_searcher, MeshGridSearcher):
        raise NotImplementedError(f"smplify.loss.{who}: mesh_grid_searcher is a {type(mesh_grid_searcher).__name__}; {_normals.FUSED_PATH}")
    if mesh_grid_searcher._scan is None:
        raise ValueError(f"{who}: the searcher has no mesh (set_mesh was not called)")
    if getattr(mesh_grid_searcher, "_mesh_wants_grad", False):
        raise ValueError(f"{who}: the scan requires grad; no gradient flows to it (the reference detaches the closest points)")
    return mesh_grid_searcher._scan


def point_cloud_loss_mesh_grid(mesh_grid_searcher, points):
    """loss.py:233-242: sqrt(sum |P - C|^2) over all of points[..., 3] with C their closest points on the searcher's mesh,
    detached.  The gradient (P - C) / loss goes to `points`, exactly zero where the loss is zero."""
    who = "point_cloud_loss_mesh_grid"
    scan = _scan_of(who, mesh_grid_searcher)
    _normals.require_array("smplify.loss." + who, "points", points)
    _prior._require_float32(who, "points", points)
    if _normals.require_rows3(who, "points", points) == 0:
        raise ValueError(f"{who}: no points")

    def call(p, want_grad):
        p = p.reshape(-1, 3)
        value, ids, nearest, grad = scan.point_loss(p, want_grad=want_grad)
        mesh_grid_searcher._remember_query(p, ids, nearest)
        return value, grad

    def device_call(p, want_grad, stream):
        import torch
        n = p.numel() // 3
        (value, grad), ids, nearest = _value_and_grad(p, want_grad), _new(p, n, torch.int32), _new(p, (n, 3))
        scan.point_loss_dev(n, stream, p.data_ptr(), loss=value.data_ptr(), face_ids=ids.data_ptr(), nearest=nearest.data_ptr(),
                            dpoints=0 if grad is None else grad.data_ptr())
        mesh_grid_searcher._remember_query_dev(points, ids, nearest)          # (the caller's tensor: what the next loss is handed)
        return value, grad

    return _scalar_loss(who, points, call, device=getattr(scan, "dev_route_device", None), device_call=device_call)


def normal_loss_mesh_grid(mesh_grid_searcher, points, face_norm_mesh=None, point_norm=None):
    """loss.py:260-271: mean(1 - sum(face_norm_mesh[closest face of points] * point_norm, -1)); face_norm_mesh[NF,3] the scan's face
    normals as the caller built them (smplify.py:149: un-normalised).  The gradient goes to `point_norm` only.  (The reference's
    parameter list; the last two have no default there.)"""
    who = "normal_loss_mesh_grid"
    scan = _scan_of(who, mesh_grid_searcher)
    named = (("points", points), ("face_norm_mesh", face_norm_mesh), ("point_norm", point_norm))
    for name, x in named:
        _normals.require_array("smplify.loss." + who, name, x)
    _normals.require_same_kind(who, named)
    for name, x in named:
        _prior._require_float32(who, name, x)
    _normals.require_no_grad(who, "face_norm_mesh", face_norm_mesh)
    rows = [_normals.require_rows3(who, name, x) for name, x in named]
    if rows[0] == 0:
        raise ValueError(f"{who}: no points")
    if rows[0] != rows[2]:
        raise ValueError(f"{who}: points has {rows[0]} rows, point_norm {rows[2]}")
    if face_norm_mesh.ndim != 2 or rows[1] != scan.n_faces:
        raise ValueError(f"{who}: face_norm_mesh must be [{scan.n_faces}, 3] (one row per face of the searcher's mesh), not {tuple(face_norm_mesh.shape)}")
    from . import native
    device = getattr(scan, "dev_route_device", None)
    if _takes_device_route(device, points, face_norm_mesh, point_norm):
        # everything is on the scan's GPU: the ids stay there (the tensor memo, or a search queued here) and the kernel gathers
        ids = mesh_grid_searcher._query_dev(points, _autograd.stream_of(points))
        table = face_norm_mesh.detach().contiguous()

        def device_call(pn, want_grad, stream):
            value, grad = _value_and_grad(pn, want_grad)
            native.normal_loss_dev(scan.workspace(), stream, rows[0], ids.data_ptr(), table.data_ptr(), scan.n_faces, pn.data_ptr(),
                                   loss=value.data_ptr(), dpoint_norms=0 if grad is None else grad.data_ptr())
            return value, grad

        return _scalar_loss(who, point_norm, None, device=device, device_call=device_call)
    ids, _ = mesh_grid_searcher._query(_host(points, None).reshape(-1, 3))
    closest = _host(face_norm_mesh, None)[ids]                 # (gathered here: N rows go up, not the scan's table)

    def call(pn, want_grad):
        return native.normal_loss(closest, pn.reshape(-1, 3), want_grad=want_grad, device=scan.device)

    return _scalar_loss(who, point_norm, call)


def normal_laplacian_smoothness(norms, faces):
    """loss.py:273-288: the mean over faces of |na-nb|^2 + |nc-na|^2 + |nb-nc|^2 of norms[..., 3].  The gradient goes to `norms`."""
    from . import native
    who = "normal_laplacian_smoothness"
    _normals.require_array("smplify.loss." + who, "norms", norms)
    _normals.require_array("smplify.loss." + who, "faces", faces)
    _normals.require_same_kind(who, (("norms", norms), ("faces", faces)))
    _prior._require_float32(who, "norms", norms)
    n = _normals.require_rows3(who, "norms", norms)
    if n == 0:
        raise ValueError(f"{who}: no normals")
    topo = _normals.topology_for(who, faces, n, _normals.device_index(norms))

    def call(a, want_grad):
        return native.normal_laplacian(topo, a.reshape(-1, 3), want_grad=want_grad)

    def device_call(a, want_grad, stream):
        value, grad = _value_and_grad(a, want_grad)
        native.normal_laplacian_dev(topo, stream, a.data_ptr(), loss=value.data_ptr(), dnorms=0 if grad is None else grad.data_ptr())
        return value, grad

    return _scalar_loss(who, norms, call, device=getattr(topo, "dev_route_device", None), device_call=device_call)


# ----------------------------------------------------------------------------------------------------------------------------
# the silhouette term (loss.py:73-130)
# ----------------------------------------------------------------------------------------------------------------------------

_SILHOUETTE_SLOTS = 4       # mask sets kept at a time; the oldest goes first
_GIVEN_SLOTS = 4            # hand-outs of extract_countours recognised per mask set
MASK_STRIDE = 4             # loss.py:99: every 4th vertex


_SILHOUETTES = {}           # a table of _memo.py: (masks, GPU, contour digest) -> sil, contours (host [C,2] arrays), given (a table of the hand-outs); dropped: closed


def _items(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _require_arrays(who, name, x):
    """an array, a tensor or a list of them; anything else: NotImplementedError (what the stand-alone stubs raised for anything)"""
    if isinstance(x, (list, tuple)):
        for it in x:
            _normals.require_array("smplify.loss." + who, f"an item of {name}", it)
    else:
        _normals.require_array("smplify.loss." + who, name, x)


def _masks_host(who, masks):
    """-> uint8 [M,H,W] of 0 / 1"""
    host = masks.detach().cpu().numpy() if _is_tensor(masks) else np.asarray(masks)
    if host.ndim == 2:
        host = host[None]
    if host.ndim != 3 or 0 in host.shape:
        raise ValueError(f"{who}: masks must be [M,H,W] (or [H,W]), not {tuple(host.shape)}")
    if not ((host == 0) | (host == 1)).all():
        raise ValueError(f"{who}: masks must hold 0 / 1 only (the reference reads them as numbers: mask < 0.1, 1 - mask)")
    return np.ascontiguousarray(host != 0, dtype=np.uint8)


def _silhouette_hit(masks, device, contour_key):
    """-> (key, the objects a look-up checks, the entry or None): like normals.topology_for"""
    seen = []
    key = (_memo.part(masks, seen), int(device), contour_key)
    return key, seen, _memo.find(_SILHOUETTES, key, seen)


def _silhouette_store(key, seen, sil, contours):
    """contours None: an object made on the device route - its host copies are fetched when something asks (_hit_contours)"""
    return _memo.store(_SILHOUETTES, _SILHOUETTE_SLOTS, key, seen, {"sil": sil, "contours": contours, "given": {}},
                       closed=lambda hit: hit["sil"].close())


def _hit_contours(hit):
    if hit["contours"] is None:
        hit["contours"] = [np.asarray(c, np.float32).reshape(-1, 2) for c in hit["sil"].contours()]
    return hit["contours"]


_MASK_DTYPES = {"torch.float32": 1, "torch.uint8": 0, "torch.bool": 0}          # -> native.MASK_FLOAT32 / MASK_UINT8


def _silhouette_offers():
    """does the library have the silhouette's device entries?  A condition of both mask routes beside _autograd.takes_device_route"""
    from . import native
    offers = getattr(native.Silhouette, "offers_dev", None)
    return offers is not None and offers()


def _masks_route(masks, device):
    """"device" when extract_countours hands `masks` to the GPU `device` by address, else "host" - never an error"""
    return "device" if _takes_device_route(device, masks, dtypes=tuple(_MASK_DTYPES)) and _silhouette_offers() else "host"


def _mask_loss_route(smpl_verts, device):
    """"device" when multview_mask_loss evaluates on GPU `device` where the vertices lie, else "host" - never an error"""
    return "device" if _silhouette_offers() and _takes_device_route(device, smpl_verts) else "host"


def _contours_on_device(sil, like):
    """the object's contours as M GPU tensors [C,1,2]: views split from ONE tensor that bf_silhouette_contours_dev fills"""
    import torch
    counts = [int(c) for c in sil.counts()]
    xy = torch.empty((max(sum(counts), 1), 2), dtype=torch.float32, device=like.device)
    sil.contours_dev(xy.data_ptr(), _autograd.stream_of(like))
    ends = np.cumsum(counts)
    return [xy[int(e) - c:int(e)].reshape(-1, 1, 2) for c, e in zip(counts, ends)]


def extract_countours(masks, device=None):
    """loss.py:73-83: masks[M,H,W] (or [H,W]; a tensor or an array of any dtype holding 0 / 1) -> a list of M float32 [C,1,2] items of
    (x, y) points in border order - OpenCV's shape - tensors on masks' device, or arrays.  Per mask the external border the
    reference keeps (loss.py:80: OpenCV's first listed contour), followed on the GPU `device` (None: masks', else 0).  The masks
    and contours stay on the GPU for the `multview_mask_loss` that follows."""
    from . import native
    who = "extract_countours"
    _normals.require_array("smplify.loss." + who, "masks", masks)
    _normals.require_no_grad(who, "masks", masks)
    if device is None:
        device = _normals.device_index(masks)
    key, seen, hit = _silhouette_hit(masks, device, None)
    on_device = _masks_route(masks, device) == "device"
    if hit is None and on_device:
        # the masks go in by address, on torch's current stream: binarised and checked by a kernel, only M + 1 flags come back
        shape = (1,) + tuple(masks.shape) if masks.ndim == 2 else tuple(masks.shape)
        if len(shape) != 3 or 0 in shape:
            raise ValueError(f"{who}: masks must be [M,H,W] (or [H,W]), not {tuple(masks.shape)}")
        m = masks.detach().contiguous()
        try:
            sil = native.Silhouette.from_device(m.data_ptr(), shape, _MASK_DTYPES[str(m.dtype)], _autograd.stream_of(m), device=device)
        except native.MasksRefused as e:
            if e.view is None:
                raise ValueError(f"{who}: masks must hold 0 / 1 only (the reference reads them as numbers: mask < 0.1, 1 - mask)") from None
            raise ValueError(f"{who}: mask {e.view} has no foreground (the reference fails in np.argmax of an empty list)") from None
        hit = _silhouette_store(key, seen, sil, None)
    if on_device and getattr(hit["sil"], "dev_route_device", None) == device:
        out = _contours_on_device(hit["sil"], masks)
        _memo.store(hit["given"], _GIVEN_SLOTS, tuple(map(id, out)), out, {})          # (recognised by identity later)
        return out
    if hit is None:
        host = _masks_host(who, masks)
        empty = [i for i in range(len(host)) if not host[i].any()]
        if empty:
            raise ValueError(f"{who}: mask {empty[0]} has no foreground (the reference fails in np.argmax of an empty list)")
        sil = native.Silhouette(host, None, device=device)           # (contour_select: OpenCV's first listed contour, the default)
        hit = _silhouette_store(key, seen, sil, [np.asarray(c, np.float32).reshape(-1, 2) for c in sil.contours()])
    out = [c.reshape(-1, 1, 2).copy() for c in _hit_contours(hit)]
    if _is_tensor(masks):
        import torch
        out = [torch.from_numpy(c).to(masks.device) for c in out]
        _memo.store(hit["given"], _GIVEN_SLOTS, tuple(map(id, out)), out, {})          # (recognised by identity later)
    return out


def _silhouette_for(who, masks, contours, device):
    """the `native.Silhouette` of (masks, contours) on GPU `device`: the one extract_countours built when these are its contours,
    else one with the caller's contours uploaded"""
    from . import native
    key, seen, hit = _silhouette_hit(masks, device, None)
    if hit is not None and hit["sil"].n_views == len(contours) and _memo.find(hit["given"], tuple(map(id, contours)), contours) is not None:
        return hit["sil"]
    known = _known_contours(masks, contours, device)
    if known is not None:
        return known
    host = []
    for i, c in enumerate(contours):
        a = _host(c)
        if a.ndim not in (2, 3) or a.shape[-1] != 2 or (a.ndim == 3 and a.shape[1] != 1):
            raise ValueError(f"{who}: contour {i} must be [C,1,2] or [C,2], not {tuple(a.shape)}")
        if a.shape[0] == 0:
            raise ValueError(f"{who}: contour {i} has no points")
        host.append(np.ascontiguousarray(a.reshape(-1, 2)))
    if hit is not None and hit["sil"].n_views == len(host) and all(np.array_equal(a, b) for a, b in zip(host, _hit_contours(hit))):
        return _remember_contours(masks, contours, device, hit["sil"])
    digest = _memo.digest(data=b"".join(a.tobytes() for a in host) + repr([len(a) for a in host]).encode())
    key, seen, hit = _silhouette_hit(masks, device, digest)
    if hit is None:
        hit = _silhouette_store(key, seen, native.Silhouette(_masks_host(who, masks), host, device=device), host)
    return _remember_contours(masks, contours, device, hit["sil"])


_KNOWN_CONTOUR_SLOTS = 4    # contour tensors that are not extract_countours' own and have been read and matched to an object once:
_KNOWN_CONTOURS = {}        # a table of _memo.py: (masks, GPU, contours) -> sil, that object; masks not held, the contours HELD


def _known_contours(masks, contours, device):
    """the object these contour TENSORS were matched to before - the same tensors at the same version beside the same masks - or
    None: a loop that passes its own contours reads them back once, not at every step.  (The tensors are held while remembered:
    an identity cannot come back with other contents.)"""
    if not (_is_tensor(masks) and all(_is_tensor(c) for c in contours)):
        return None
    hit = _memo.find(_KNOWN_CONTOURS, (id(masks), device, tuple(map(id, contours))), [masks, *contours])
    cached = hit is not None and any(h["sil"] is hit["sil"] for h in _SILHOUETTES.values())          # (not closed by an eviction)
    return hit["sil"] if cached else None


def _remember_contours(masks, contours, device, sil):
    if _is_tensor(masks) and all(_is_tensor(c) for c in contours):
        _memo.store(_KNOWN_CONTOURS, _KNOWN_CONTOUR_SLOTS, (id(masks), device, tuple(map(id, contours))), [masks, *contours], {"sil": sil},
                    hold=[False] + [True] * len(contours))
    return sil


_CAMERA_SLOTS = 4           # camera sets kept at a time; the oldest goes first
_CAMERAS = {}               # a table of _memo.py: (device, camera objects) -> w2c, K stacked there; the objects are HELD: their ids are the key
CAMERA_STATS = {"stacks": 0}          # how often a camera set was stacked on a GPU (the tests read it)


def _cameras_for(who, cameras, n_views, torch_device):
    """w2cs, Ks (each one stacked tensor, or a list of tensors) as float32 [M,4,4] and [M,3,3] on `torch_device`: stacked there once
    per distinct set - its items by identity and version, like _views_for - and remembered.  GPU cameras are never read back;
    CPU tensors are sent once per set."""
    import torch
    items = [x if _is_tensor(x) else list(x) for x in cameras]
    flat = [it for x in items for it in ([x] if _is_tensor(x) else x)]
    key = (torch_device, n_views, tuple(len(x) if isinstance(x, list) else -1 for x in items), tuple(map(id, flat)))
    hit = _memo.find(_CAMERAS, key, flat)
    if hit is None:
        out = []
        try:
            for x, side in zip(items, (4, 3)):
                x = x.detach() if _is_tensor(x) else torch.stack([t.detach().reshape(side, side) for t in x])
                out.append(x.reshape(n_views, side, side).to(device=torch_device, dtype=torch.float32).contiguous())
        except RuntimeError:
            raise ValueError(f"{who}: w2cs must be [M,4,4] and Ks [M,3,3]") from None
        CAMERA_STATS["stacks"] += 1
        hit = _memo.store(_CAMERAS, _CAMERA_SLOTS, key, flat, {"w2c": out[0], "K": out[1]}, hold=True)
    return hit["w2c"], hit["K"]


def multview_mask_loss(contours, masks, smpl_verts=None, smpl_faces=None, w2cs=None, Ks=None, mask_frames=None, epsilon=10, imsize=512,
                       device=None, pairwise=None):
    """loss.py:85-130, the reference's parameters in its order (from the third on they have no default there) plus `device` (the
    GPU; None: smpl_verts', else 0) and `pairwise` (None or 'cdist': distances in torch.cdist's float32 form, as the reference and
    SMPLify compute them; 'exact': (a - b)^2 sums).  contours: M items [C,1,2] or [C,2]; masks[M,H,W] of 0 / 1; smpl_verts[1,N,3]
    or [N,3] float32 - every 4th vertex is used; smpl_faces is accepted and ignored (the reference only converts it); w2cs[M,4,4],
    Ks[M,3,3] (tensors, arrays or lists of them); of mask_frames only the length is read.  -> the unweighted loss: a 0-dim float32
    tensor on smpl_verts' device, differentiable once with respect to smpl_verts, or a float for arrays.  A view none of whose
    sampled vertices lies inside the image contributes its binary term only (the reference raises in torch.min)."""
    who = "multview_mask_loss"
    named = (("contours", contours), ("masks", masks), ("smpl_verts", smpl_verts), ("w2cs", w2cs), ("Ks", Ks))
    for name, x in named:
        _require_arrays(who, name, x)
    if isinstance(masks, (list, tuple)) or isinstance(smpl_verts, (list, tuple)):
        raise ValueError(f"{who}: masks and smpl_verts must be one tensor or array each, not a list")
    flat = [(name, it) for name, x in named for it in _items(x)]
    if len({_is_tensor(it) for _, it in flat}) > 1:
        raise ValueError(f"{who}: the arguments mix torch tensors and numpy arrays")
    for name, it in flat:
        if name != "smpl_verts":
            _normals.require_no_grad(who, name, it)
    _prior._require_float32(who, "smpl_verts", smpl_verts)
    if smpl_verts.ndim not in (2, 3) or smpl_verts.shape[-1] != 3 or (smpl_verts.ndim == 3 and smpl_verts.shape[0] != 1) or smpl_verts.shape[-2] == 0:
        raise ValueError(f"{who}: smpl_verts must be [1,N,3] or [N,3], not {tuple(smpl_verts.shape)}")
    if mask_frames is None:
        raise ValueError(f"{who}: mask_frames is missing (its length is the number of views)")
    n_masks = 1 if masks.ndim == 2 else len(masks)
    cameras_given = (w2cs, Ks)
    contours, w2cs, Ks = list(contours), list(w2cs), list(Ks)
    if not (len(mask_frames) == n_masks == len(contours) == len(w2cs) == len(Ks)):
        raise ValueError(f"{who}: {len(mask_frames)} mask_frames, {n_masks} masks, {len(contours)} contours, {len(w2cs)} w2cs and {len(Ks)} Ks "
                         "(the reference fails in .view)")
    if masks.ndim not in (2, 3):
        raise ValueError(f"{who}: masks must be [M,H,W], not {tuple(masks.shape)}")
    imsize, epsilon = float(imsize), float(epsilon)
    if not np.isfinite(epsilon):
        raise ValueError(f"{who}: epsilon must be finite")
    if not (np.isfinite(imsize) and imsize > 0):
        raise ValueError(f"{who}: imsize must be finite and positive")
    if imsize > min(masks.shape[-2:]):
        raise ValueError(f"{who}: imsize {imsize:g} is larger than the masks ({masks.shape[-2]} x {masks.shape[-1]}): the reference indexes "
                         "beyond the mask as soon as a chosen vertex lies there")
    if pairwise not in (None, "cdist", "exact"):
        raise ValueError(f"{who}: pairwise must be None, 'cdist' or 'exact'")
    if device is None:
        device = _normals.device_index(smpl_verts)
    if _mask_loss_route(smpl_verts, device) == "device":
        # float32 vertices on the GPU: everything stays there.  The cameras are stacked on that GPU once per distinct set, the
        # contours are recognised by identity (else built through the host, once per set), the loss is a tensor that never leaves
        w2c_t, K_t = _cameras_for(who, cameras_given, n_masks, smpl_verts.device)
        sil = _silhouette_for(who, masks, contours, device)
        if getattr(sil, "dev_route_device", None) == device:
            def device_call(v, want_grad, stream):
                terms, grad = _value_and_grad(v, want_grad, 1 + 2 * n_masks)
                sil.loss_dev(stream, v.numel() // 3, v.data_ptr(), w2c_t.data_ptr(), K_t.data_ptr(), imsize=imsize, epsilon=epsilon,
                             stride=MASK_STRIDE, cdist_form=pairwise != "exact", terms=terms.data_ptr(),
                             dverts=0 if grad is None else grad.data_ptr())
                return terms[:1], grad

            return _scalar_loss(who, smpl_verts, None, plus_zero=True, device=device, device_call=device_call)
    try:
        w2c = np.stack([_host(a).reshape(4, 4) for a in w2cs])
        K = np.stack([_host(a).reshape(3, 3) for a in Ks])
    except ValueError:
        raise ValueError(f"{who}: w2cs must be [M,4,4] and Ks [M,3,3]") from None
    sil = _silhouette_for(who, masks, contours, device)

    def call(v, want_grad):
        value, _, grad = sil.loss(v.reshape(-1, 3), w2c, K, imsize=imsize, epsilon=epsilon, stride=MASK_STRIDE,
                                  cdist_form=pairwise != "exact", want_grad=want_grad)
        return value, grad

    return _scalar_loss(who, smpl_verts, call, plus_zero=True)


# ----------------------------------------------------------------------------------------------------------------------------
# multiview_keypoint_loss (loss.py:139-230)
# ----------------------------------------------------------------------------------------------------------------------------

def _no_grad_input(name, x):
    items = x if isinstance(x, (list, tuple)) else [x]
    for it in items:
        values = it.values() if isinstance(it, dict) else [it]
        if any(_is_tensor(v) and v.requires_grad for v in values):
            raise ValueError(f"multiview_keypoint_loss: {name} requires grad; gradients flow to model_joints, poses and betas only")


_VIEW_SLOTS = 4             # view sets kept at a time; the oldest goes first
_VIEWS = {}                 # a table of _memo.py: cameras and keypoints -> host (w2c, K, kp, present), dev {gpu: the four as tensors}; tensors not held
VIEW_STATS = {"packs": 0, "uploads": 0}          # how often a view set was packed on the host / sent to a GPU (the tests read them)


def _views_key(w2cs, Ks, keypoints, n_use, use_hand_face, rows):
    """-> (key, the tensors a look-up checks): like _silhouette_hit, a tensor by identity and version, anything else by a digest of its
    contents"""
    seen = []

    def one(a):
        return None if a is None else _memo.part(a, seen)

    def entry(k):                # (by part name, whatever order the dict was filled in: `seen` is collected in the key's order)
        return None if k is None else tuple((part, one(a)) for part, a in sorted(k.items()))

    def cameras(x):              # (a stacked tensor is one object: its rows would be new views at every call)
        return one(x) if _is_tensor(x) else tuple(one(x[i]) for i in range(min(n_use, len(x))))

    key = (n_use, bool(use_hand_face), rows, cameras(w2cs), cameras(Ks), tuple(entry(keypoints[i]) for i in range(min(n_use, len(keypoints)))))
    return key, seen


def _views_for(w2cs, Ks, keypoints, n_use, use_hand_face, rows):
    """the packed views of this call: remembered ones when the same cameras and keypoints come again, else packed now"""
    try:
        key, seen = _views_key(w2cs, Ks, keypoints, n_use, use_hand_face, rows)
    except (TypeError, AttributeError):          # (something that is neither: packed every time, as before)
        return {"host": _pack_views(w2cs, Ks, keypoints, n_use, use_hand_face, rows), "dev": {}}
    hit = _memo.find(_VIEWS, key, seen)
    if hit is not None:
        return hit
    packed = _pack_views(w2cs, Ks, keypoints, n_use, use_hand_face, rows)
    VIEW_STATS["packs"] += 1
    return _memo.store(_VIEWS, _VIEW_SLOTS, key, seen, {"host": packed, "dev": {}})


def _views_on(views, device):
    """the four packed arrays as tensors on that GPU, sent on first use"""
    import torch
    if device not in views["dev"]:
        # (contiguous first: cameras from torch.inverse arrive column-major, np.stack keeps that order, and a tensor made from such an
        # array keeps its strides - the kernel reads by address and would see every w2c transposed)
        views["dev"][device] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in views["host"])
        VIEW_STATS["uploads"] += 1
    return views["dev"][device]


class _DeviceRoute:
    """`native.keypoint_loss` on tensors of the prior's GPU (_autograd.apply's device_route): inputs (joints, poses, betas), output terms"""

    def __init__(self, views, n_use, gmm, hyper, device):
        self.views, self.n_use, self.gmm, self.hyper, self.device = views, n_use, gmm, hyper, int(device)

    def _call(self, x, stream, **out):
        from . import native
        j, p, b = x
        w2c, K, kp, present = _views_on(self.views, j.device)
        native.keypoint_loss_dev(stream, 1, rows=j.shape[1], joints=j.data_ptr(), n_views=self.n_use, w2c=w2c.data_ptr(), K=K.data_ptr(),
                                 keypoints=kp.data_ptr(), present=present.data_ptr(), divisor=[self.n_use], pose_dim=p.shape[-1],
                                 poses=p.data_ptr(), n_betas=b.shape[-1], betas=b.data_ptr(), gmm=self.gmm, hyper=self.hyper,
                                 device=self.device, **{k: v.data_ptr() for k, v in out.items() if v is not None})

    def forward(self, x, stream):
        import torch
        terms = torch.empty((1, 4), dtype=torch.float32, device=x[0].device)
        self._call(x, stream, terms=terms)
        return (terms,)

    def vjp(self, x, cotangents, want, stream):
        import torch
        grads = [torch.empty_like(t) if w else None for t, w in zip(x, want)]
        self._call(x, stream, dterms=cotangents[0], djoints=grads[0], dposes=grads[1], dbetas=grads[2])
        return grads


def _pack_views(w2cs, Ks, keypoints, n_use, use_hand_face, rows):
    """-> w2c[1,V,4,4], K[1,V,3,3], kp[1,V,rows,3], present[1,V] over the V = len(use_frames) views the reference loops over"""
    if len(keypoints) < n_use or len(w2cs) < n_use or len(Ks) < n_use:
        raise ValueError(f"multiview_keypoint_loss: {n_use} use_frames but fewer cameras or keypoint entries")
    w2c = np.stack([_host(w2cs[i]).reshape(4, 4) for i in range(n_use)])[None]
    K = np.stack([_host(Ks[i]).reshape(3, 3) for i in range(n_use)])[None]
    kp = np.zeros((1, n_use, rows, 3), np.float32)
    present = np.zeros((1, n_use), np.uint8)
    groups = {"hand": False, "face": False}
    for i in range(n_use):
        k = keypoints[i]
        if k is None:                                              # loss.py:157
            continue
        present[0, i] = 1
        if use_hand_face:
            # (hands and face: every joint of a part weighted by the part's summed squared confidences, loss.py:168-181 - keypoints.py)
            kp[0, i] = pack_keypoints_smplx({part: _host(a) for part, a in k.items()})
            groups["hand"] |= "hand_left" in k or "hand_right" in k
            groups["face"] |= "face" in k
        else:
            kp[0, i] = _host(k["pose"])[:SKELETON_LENGTH]
    if not present.any():
        raise ValueError("multiview_keypoint_loss: no view has keypoints (the reference fails in torch.stack)")
    if use_hand_face:
        for name, seen in groups.items():
            if not seen:
                raise ValueError(f"multiview_keypoint_loss: use_hand_face with no {name} keypoints in any view (the reference fails in torch.stack)")
    return w2c, K, kp, present


def multiview_keypoint_loss(w2cs, Ks, keypoints, model_joints, poses, betas, use_frames, pose_prior, sigma=100,
                            shape_prior_weight=5, angle_prior_weight=15.2, output='sum', debug=False, imsize=512,
                            pose_prior_weight=4.78, use_hand_face=False, output_folder=None, verts=None, device=None):
    """The reference's signature plus `device` (the GPU; None: the prior's, else 0).  w2cs[V,4,4], Ks[V,3,3] (tensors, arrays or
    lists of them), keypoints: per view None or the OpenPose dict ('pose', with use_hand_face optionally 'hand_left', 'hand_right',
    'face'), model_joints[1,J,3] (the first 25 are compared; with use_hand_face J = 135), poses[1,69] (63 with use_hand_face),
    betas[1,NB].  pose_prior: this project's MaxMixturePrior, any object with means / precisions / nll_weights, or another
    callable (called as pose_prior(poses69, None) outside the kernel).  -> (total, {four terms as host values}).
    debug, output_folder and verts are accepted and ignored (their use is commented out in the reference)."""
    from . import native
    if output != 'sum':
        raise ValueError("multiview_keypoint_loss: only output='sum' is supported (the reference returns a function object otherwise)")
    tensors = any(_is_tensor(x) for x in (model_joints, poses, betas))
    for name, x in (("model_joints", model_joints), ("poses", poses), ("betas", betas)):
        if tensors and not _is_tensor(x):
            raise ValueError(f"multiview_keypoint_loss: {name} is not a tensor while others are")
        _prior._require_float32("multiview_keypoint_loss", name, x)
    for name, x in (("w2cs", w2cs), ("Ks", Ks), ("keypoints", [k for k in keypoints if k is not None])):
        _no_grad_input(name, x)
    if model_joints.ndim != 3 or model_joints.shape[0] != 1 or poses.shape[0] != 1 or betas.shape[0] != 1:
        raise ValueError("multiview_keypoint_loss: batch size must be 1 (the reference projects row 0 only)")
    rows = SKELETON_LENGTH + HANDS_LENGTH + FACE_LENGTH if use_hand_face else SKELETON_LENGTH
    if model_joints.shape[1] < rows or (use_hand_face and model_joints.shape[1] != rows):
        raise ValueError(f"multiview_keypoint_loss: model_joints has {model_joints.shape[1]} joints, {rows} are compared")
    n_use = len(use_frames)
    views = _views_for(w2cs, Ks, keypoints, n_use, use_hand_face, rows)
    w2c, K, kp, present = views["host"]
    divisor = np.array([n_use], np.int32)

    gmm, generic = None, None
    if isinstance(pose_prior, _prior.MaxMixturePrior) or _prior.is_gmm_like(pose_prior):
        gmm = _prior.device_gmm(pose_prior, device)
    elif callable(pose_prior):
        generic = pose_prior
    else:
        raise ValueError("multiview_keypoint_loss: pose_prior must be a MaxMixturePrior, an object with its buffers, or a callable")
    if device is None:
        device = gmm.device if gmm is not None else 0
    hyper = native.make_hyper(sigma=sigma, shape_prior_weight=shape_prior_weight, angle_prior_weight=angle_prior_weight,
                              pose_prior_weight=pose_prior_weight, imsize=imsize)
    common = dict(w2c=w2c, K=K, keypoints=kp, present=present, divisor=divisor, gmm=gmm, hyper=hyper, device=device)

    def forward(j, p, b):
        return (native.keypoint_loss(j, poses=p, betas=b, want=("terms",), **common)["terms"],)

    def vjp(arrays, cotangents):
        j, p, b = arrays
        out = native.keypoint_loss(j, poses=p, betas=b, dterms=cotangents[0], want=("djoints", "dposes", "dbetas"), **common)
        return out["djoints"], out["dposes"], out["dbetas"]

    w2 = pose_prior_weight ** 2
    if not tensors:
        terms = forward(np.asarray(model_joints)[:, :rows], np.asarray(poses), np.asarray(betas))[0][0]
        losses = {k: float(terms[i]) for i, k in enumerate(LOSS_KEYS)}
        if generic is not None:
            p69 = np.concatenate([np.asarray(poses), np.zeros_like(np.asarray(poses)[:, :6])], -1) if use_hand_face else np.asarray(poses)
            losses["pose_prior_loss"] = float(w2 * np.asarray(_host(generic(p69, None))).reshape(-1)[0])
        return float(sum(losses.values())), losses

    import torch
    inputs = (model_joints[:, :rows], poses, betas)
    route = _DeviceRoute(views, n_use, gmm, hyper, device)
    terms = _autograd.apply(forward, vjp, inputs, device_route=route)[0]
    if _autograd.chosen_route(inputs, route) == "device":
        # the four terms added in the order torch's CPU sum adds them, ((a + b) + c) + d: a GPU reduction pairs them otherwise, and
        # the total of a GPU call would differ from the CPU call's in its last bit
        a, b, c, d = terms[0].unbind(0)
        total = ((a + b) + c) + d
    else:
        total = terms.sum()
    host = terms.detach().cpu().numpy()
    losses = {"reprojection_loss": host[0, 0], "pose_prior_loss": host[:, 1], "angle_prior_loss": host[:, 2], "shape_prior_loss": host[:, 3]}
    if generic is not None:
        p69 = torch.cat([poses, torch.zeros_like(poses[:, :6])], dim=-1) if use_hand_face else poses          # loss.py:206-207
        extra = w2 * generic(p69, None)
        total = total + extra.sum()
        losses["pose_prior_loss"] = extra.detach().cpu().numpy()
    return total, losses
