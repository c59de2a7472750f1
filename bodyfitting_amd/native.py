"""Thin numpy-level wrappers over the C ABI: `DeviceModel` (bf_model) and `FrameBatch` (bf_batch).

Host code is plain Python + numpy + ctypes; PyTorch is not involved on this path.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from .assets import gmm_buffers
from .keypoints import pack_keypoints_smplx

N_LOSS_JOINTS = 25   # SKELETON_LENGTH, reference smplify/loss.py:17


def _f32(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


_F32, _I32 = np.dtype(np.float32), np.dtype(np.int32)


def conforming_address(a, dtype, size):
    """the address of `a` if it already is what the library reads - an ndarray of `dtype`, C-contiguous, `size` elements - else None.
    Nothing is converted, copied or kept: the caller's array outlives the call it is passed to."""
    if type(a) is np.ndarray and (a.dtype is dtype or a.dtype == dtype) and a.size == size and a.flags.c_contiguous:
        try:
            return C.addressof(C.c_char.from_buffer(a))         # (the buffer protocol: a third of the time a.ctypes takes)
        except (TypeError, ValueError):                         # a read-only or an empty array
            return a.ctypes.data
    return None


def stage_addresses(F, n_kp, n_betas, keypoints, n_use_frames, init_betas, init_pose):
    """stage_inputs' arguments as four addresses when all of them conform (n_use_frames: None, or int32[F]), else None"""
    kp = conforming_address(keypoints, _F32, n_kp)
    b = conforming_address(init_betas, _F32, F * n_betas)
    p = conforming_address(init_pose, _F32, F * 72)
    nd = None if n_use_frames is None else conforming_address(n_use_frames, _I32, F)
    if kp is None or b is None or p is None or (nd is None and n_use_frames is not None):
        return None
    return kp, nd, b, p


def model_desc(model, gmm):
    """-> (ModelDesc for bf_model_create / bf_group_create, dict of the model's sizes, the arrays the descriptor points into -
    keep them alive until the call returned)."""
    model_type = model.get("model_type", "smpl")
    means, prec, nllw = gmm_buffers(gmm) if isinstance(gmm, dict) else gmm
    smplx = model_type == "smplx"
    # SMPL-X: the 10 core shape directions go into the descriptor; the columns behind them - shape directions from the eleventh to
    # the dict's "num_betas" (absent: 10), then the expression directions - are attached apart by DeviceModel
    # (bf_model_set_expression / bf_model_set_shape_space): the fit optimises the ten core betas and nothing else
    n_betas = 10 if smplx else np.asarray(model["shapedirs"]).shape[2]
    num_betas = int(model.get("num_betas", 10)) if smplx else n_betas
    if smplx and not 10 <= num_betas <= np.asarray(model["shapedirs"]).shape[2]:
        raise ValueError(f"num_betas={num_betas}: an SMPL-X model dict holds 10 .. shapedirs.shape[2] = {np.asarray(model['shapedirs']).shape[2]} shape directions")
    if "J_regressor_extra" not in model:
        model = dict(model, J_regressor_extra=np.zeros((0, np.asarray(model["v_template"]).shape[0]), np.float32))
    keep = {
        "v_template": _f32(model["v_template"]), "shapedirs": _f32(np.asarray(model["shapedirs"])[:, :, :n_betas]),
        "posedirs": _f32(model["posedirs"]), "j_regressor": _f32(model["J_regressor"]),
        "lbs_weights": _f32(model["lbs_weights"]), "parents": _i32(model["parents"]),
        "selector_ids": _i32(model["selector_ids"]),
        "j_regressor_extra": _f32(model["J_regressor_extra"]), "joint_map": _i32(model["joint_map"]),
        "gmm_means": _f32(means), "gmm_precisions": _f32(prec), "gmm_nll_weights": _f32(nllw),
    }
    info = {"model_type": model_type}
    info["n_verts"], info["n_joints"] = keep["lbs_weights"].shape
    info["n_betas"] = keep["shapedirs"].shape[2]           # the descriptor's: what the fit and the packed parameter vector carry
    info["num_betas"] = num_betas                          # what the stand-alone smplx calls take (DeviceModel.n_betas)
    info["n_selector"] = len(keep["selector_ids"])
    info["n_joint_map"] = len(keep["joint_map"])
    info["faces"] = _i32(model["faces"]) if "faces" in model else None
    if keep["posedirs"].shape != (9 * (info["n_joints"] - 1), 3 * info["n_verts"]):
        raise ValueError("posedirs must be [9(NJ-1), 3NV] as smplx stores it")
    d = _lib.ModelDesc()
    d.n_verts, d.n_joints, d.n_betas = info["n_verts"], info["n_joints"], info["n_betas"]
    for name in ("v_template", "shapedirs", "posedirs", "j_regressor", "lbs_weights", "j_regressor_extra",
                 "gmm_means", "gmm_precisions", "gmm_nll_weights"):
        setattr(d, name, _lib.fptr(keep[name]))
    for name in ("parents", "selector_ids", "joint_map"):
        setattr(d, name, _lib.iptr(keep[name]))
    d.n_selector, d.n_extra = info["n_selector"], keep["j_regressor_extra"].shape[0]
    info["n_loss_joints"] = 135 if smplx else N_LOSS_JOINTS               # loss.py:17-19: 25 (+ 42 hands + 68 face)
    d.n_joint_map, d.n_loss_joints = info["n_joint_map"], info["n_loss_joints"]
    if smplx:
        keep.update(pose_mean=_f32(model["pose_mean"]), lhc=_f32(model["left_hand_components"]),
                    rhc=_f32(model["right_hand_components"]), lmk_f=_i32(model["lmk_faces_idx"]),
                    lmk_b=_f32(model["lmk_bary_coords"]), dyn_f=_i32(model["dynamic_lmk_faces_idx"]),
                    dyn_b=_f32(model["dynamic_lmk_bary_coords"]))
        d.model_kind, d.pose_mean, d.n_hand_pca = 1, _lib.fptr(keep["pose_mean"]), keep["lhc"].shape[0]
        d.left_hand_components, d.right_hand_components = _lib.fptr(keep["lhc"]), _lib.fptr(keep["rhc"])
        d.n_lmk_static, d.lmk_faces_idx, d.lmk_bary_coords = len(keep["lmk_f"]), _lib.iptr(keep["lmk_f"]), _lib.fptr(keep["lmk_b"])
        d.n_dyn_rows, d.n_lmk_dynamic = keep["dyn_f"].shape
        d.dynamic_lmk_faces_idx, d.dynamic_lmk_bary_coords = _lib.iptr(keep["dyn_f"]), _lib.fptr(keep["dyn_b"])
        d.neck_joint = int(np.asarray(model["neck_kin_chain"])[0])
        info["n_hand_pca"] = keep["lhc"].shape[0]
        if np.asarray(model["shapedirs"]).shape[2] > n_betas:
            keep["exprdirs"] = _f32(np.asarray(model["shapedirs"])[:, :, n_betas:])
        # all joints smplx returns before a joint_mapper: chain | selector vertices | extra regressor rows | 51 + 17 landmarks
        info["n_joints_all"] = info["n_joints"] + info["n_selector"] + keep["j_regressor_extra"].shape[0] + len(keep["lmk_f"]) + keep["dyn_f"].shape[1]
    d.gmm_components, d.gmm_dim = keep["gmm_means"].shape
    if info["faces"] is not None:
        keep["faces"] = _i32(info["faces"].reshape(-1, 3))
        d.n_faces, d.faces = len(keep["faces"]), _lib.iptr(keep["faces"])
    return d, info, keep


class Workspace:
    """The scratch of one caller of the device route (bf_workspace): grow-only device buffers and one event on GPU `device`.
    One call at a time: the *_dev wrappers hold `lock` around theirs."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self.device = int(device)
        self.lock = threading.Lock()
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_workspace_create(self.device, C.byref(self._h)), "bf_workspace_create")

    def close(self):
        if getattr(self, "_h", None):
            with self.lock:
                self._lib.bf_workspace_destroy(self._h)
                self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def device_pointer_check(device, address):
    """does the library's HIP runtime know `address` as memory of GPU `device` (bf_device_pointer_check) - in a torch process: do
    torch and the library share one runtime, so that a tensor's data_ptr() and a stream's handle mean something in here"""
    return _lib.load().bf_device_pointer_check(int(device), C.c_void_p(address or None)) == 0


def dev_route_stats():
    """bf_dev_route_stats -> dict(host_calls, dev_calls, allocations, stream_switches), process-wide"""
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load().bf_dev_route_stats(out), "bf_dev_route_stats")
    return dict(zip(("host_calls", "dev_calls", "allocations", "stream_switches"), (int(v) for v in out)))


# the device route of the SMPL+D stage's losses and of the closest-point search (bf_*_dev of csrc/mesh_loss_api.hip)
MESH_LOSS_DEV_SYMBOLS = ("bf_vertex_normals_dev", "bf_vertex_normals_vjp_dev", "bf_normal_laplacian_dev", "bf_scan_point_loss_dev",
                         "bf_scan_nearest_dev", "bf_normal_loss_dev", "bf_scale_gradient_dev")


def offers_mesh_loss_dev(lib):
    """does the library `lib` export every entry point of that route?  One without them offers no device route there: `Topology` and
    `Scan` then say `dev_route_device` None and everything takes the host route"""
    return all(hasattr(lib, name) for name in MESH_LOSS_DEV_SYMBOLS)


def _own_workspace(obj):
    """the `Workspace` of `obj` (a DeviceModel, a Gmm, a Topology, a Scan, a Silhouette), made on first use and closed with it"""
    ws = obj.__dict__.get("_workspace")
    if ws is None:
        ws = obj.__dict__.setdefault("_workspace", Workspace(obj.device))
    return ws


def _close_workspace(obj):
    """... closed BEFORE the object's own buffers go: closing drains the stream of the workspace's last call, behind which every
    earlier call on the object is ordered"""
    ws = obj.__dict__.pop("_workspace", None)
    if ws is not None:
        ws.close()


class DeviceModel:
    """Body model + GMM prior uploaded once to one GPU (replaces the per-frame construction at
    reference smplify/body_fitting.py:82 -> smplify/smplify.py:46-56).  An SMPL-X model dict whose shapedirs has more than
    10 columns brings its expression directions (columns 10:), n_expression of them; 0 otherwise.  A dict with "num_betas" > 10 has
    that many shape directions in front of them: `n_betas` is then that total - the width of forward_smplx's / vjp_smplx's betas -
    while the fit and the packed parameter vector keep the first `n_core_betas` = 10."""

    dtype = np.float32          # what the kernels compute in

    def __init__(self, model, gmm, device=0):
        lib = _lib.load()
        self._lib = lib
        d, info, keep = model_desc(model, gmm)
        self.__dict__.update(info)
        self._h = C.c_void_p()
        _lib.check(lib.bf_model_create(C.byref(d), int(device), C.byref(self._h)), "bf_model_create")
        self.n_core_betas = self.n_betas
        if "exprdirs" in keep:              # an SMPL-X model dict whose shapedirs has more than 10 columns: the shape directions from the eleventh on, then the expression directions
            n_ext = keep["exprdirs"].shape[2]
            n_expr = n_ext - (self.num_betas - self.n_core_betas)
            if self.num_betas == self.n_core_betas and n_expr <= 16:
                _lib.check(lib.bf_model_set_expression(self._h, n_expr, _lib.fptr(keep["exprdirs"])), "bf_model_set_expression")
            else:
                _lib.check(lib.bf_model_set_shape_space(self._h, self.num_betas, n_expr, _lib.fptr(keep["exprdirs"])), "bf_model_set_shape_space")
        self.n_expression = lib.bf_model_n_expression(self._h)
        self.n_betas = lib.bf_model_n_betas(self._h)
        self.shape_ext_wide = bool(lib.bf_model_shape_ext_wide(self._h))       # the directions run on shape_ext_kernels.hip
        del keep
        self.device = int(device)
        self.n_params = lib.bf_model_n_params(self._h)
        self.fit_instance = "sized" if lib.bf_model_fit_instance(self._h) else "table-driven"

    def sub_vertices(self, which):
        """full-model vertex ids of a sub-model of the dense iterations, in its order (bf_model_sub_vertices): which = 0 the
        sampled-first one, 1 the keypoint-only one; an empty array when the model has none"""
        n = self._lib.bf_model_sub_vertices(self._h, int(which), None)
        if n < 0:
            _lib.check(n, "bf_model_sub_vertices")
        ids = np.empty(n, np.int32)
        if n:
            self._lib.bf_model_sub_vertices(self._h, int(which), _lib.iptr(ids))
        return ids

    def close(self):
        _close_workspace(self)
        if getattr(self, "_h", None):
            self._lib.bf_model_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def workspace(self):
        """the model's own `Workspace` for the device route, made on first use and closed with the model"""
        return _own_workspace(self)

    # The device route (bf_*_dev): the four calls below on device ADDRESSES (integers, e.g. a tensor's data_ptr(); 0 / None = NULL)
    # of contiguous float32 arrays on the model's GPU, queued on `stream` (a hipStream_t handle, 0: the null stream).  They return
    # when the work is queued; the arrays must outlive it on that stream.  ws: a `Workspace` (None: the model's own).

    def forward_dev(self, n, stream, betas, global_orient, body_pose, vertices=0, joints=0, joints_ori=0, ws=None):
        """`forward` into vertices[n,NV,3], joints[n,n_joint_map,3], joints_ori[n,NJ+n_selector,3] (bf_smpl_forward_dev)"""
        ws = ws or self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_smpl_forward_dev(self._h, ws._h, stream or None, int(n), betas or None, global_orient or None,
                                                     body_pose or None, vertices or None, joints or None, joints_ori or None),
                       "bf_smpl_forward_dev")

    def vjp_dev(self, n, stream, betas, global_orient, body_pose, dverts=0, djoints=0, djoints_ori=0, dbetas=0, dglobal_orient=0,
                dbody_pose=0, ws=None):
        """`vjp` into dbetas[n,NB], dglobal_orient[n,3], dbody_pose[n,3(NJ-1)]; a gradient left 0 is not computed (bf_smpl_vjp_dev)"""
        ws = ws or self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_smpl_vjp_dev(self._h, ws._h, stream or None, int(n), betas or None, global_orient or None,
                                                 body_pose or None, dverts or None, djoints or None, djoints_ori or None,
                                                 dbetas or None, dglobal_orient or None, dbody_pose or None), "bf_smpl_vjp_dev")

    def forward_smplx_dev(self, n, stream, params, expression=0, vertices=0, joints=0, joints_all=0, full_pose=0, dyn_row=0, ws=None):
        """`forward_smplx` (bf_smplx_forward_dev): params = the eight addresses in forward_smplx's order (the optional five may be
        0); dyn_row: an int32[n] array"""
        ws = ws or self.workspace()
        par = _lib.SmplxParams(*[_lib.at(a) for a in params])
        out = _lib.SmplxOutputs(_lib.at(vertices), _lib.at(joints), _lib.at(joints_all), _lib.at(full_pose), _lib.at(dyn_row, _lib._IP))
        with ws.lock:
            _lib.check(self._lib.bf_smplx_forward_dev(self._h, ws._h, stream or None, int(n), C.byref(par), expression or None,
                                                      C.byref(out)), "bf_smplx_forward_dev")

    def vjp_smplx_dev(self, n, stream, params, expression=0, dverts=0, djoints=0, djoints_all=0, dfull_pose=0, grads=(0,) * 8,
                      dexpression=0, ws=None):
        """`vjp_smplx` (bf_smplx_vjp_dev): grads = the eight destination addresses in the parameters' order (0: not wanted)"""
        ws = ws or self.workspace()
        par = _lib.SmplxParams(*[_lib.at(a) for a in params])
        cot = _lib.SmplxCotangents(*[_lib.at(a) for a in (dverts, djoints, djoints_all, dfull_pose)])
        dst = _lib.SmplxGrads(*[_lib.at(a) for a in grads])
        with ws.lock:
            _lib.check(self._lib.bf_smplx_vjp_dev(self._h, ws._h, stream or None, int(n), C.byref(par), expression or None,
                                                  C.byref(cot), C.byref(dst), dexpression or None), "bf_smplx_vjp_dev")

    def forward(self, betas, global_orient, body_pose):
        """models.smpl.SMPL.forward (reference models/smpl.py:69-83): -> vertices, joints49, joints45."""
        betas = _f32(betas, (-1, self.n_betas))
        n = betas.shape[0]
        orient = _f32(global_orient, (n, 3))
        pose = _f32(body_pose, (n, 3 * (self.n_joints - 1)))
        verts = np.empty((n, self.n_verts, 3), np.float32)
        joints = np.empty((n, self.n_joint_map, 3), np.float32)
        jori = np.empty((n, self.n_joints + self.n_selector, 3), np.float32)
        _lib.check(self._lib.bf_smpl_forward(self._h, n, _lib.fptr(betas), _lib.fptr(orient), _lib.fptr(pose),
                                             _lib.fptr(verts), _lib.fptr(joints), _lib.fptr(jori)), "bf_smpl_forward")
        return verts, joints, jori

    def vjp(self, betas, global_orient, body_pose, dverts=None, djoints=None, djoints_ori=None):
        """The backward of `forward` (bf_smpl_vjp): cotangents of vertices[n,NV,3], joints[n,n_joint_map,3] and
        joints_ori[n,NJ+n_selector,3] (None = zero) -> dbetas[n,NB], dglobal_orient[n,3], dbody_pose[n,3(NJ-1)].
        SMPL-kind models only."""
        betas = _f32(betas, (-1, self.n_betas))
        n = betas.shape[0]
        orient = _f32(global_orient, (n, 3))
        pose = _f32(body_pose, (n, 3 * (self.n_joints - 1)))
        dv = None if dverts is None else _f32(dverts, (n, self.n_verts, 3))
        dj = None if djoints is None else _f32(djoints, (n, self.n_joint_map, 3))
        djo = None if djoints_ori is None else _f32(djoints_ori, (n, self.n_joints + self.n_selector, 3))
        dbetas = np.empty((n, self.n_betas), np.float32)
        dorient = np.empty((n, 3), np.float32)
        dpose = np.empty((n, 3 * (self.n_joints - 1)), np.float32)
        _lib.check(self._lib.bf_smpl_vjp(self._h, n, _lib.fptr(betas), _lib.fptr(orient), _lib.fptr(pose), _lib.fptr(dv),
                                         _lib.fptr(dj), _lib.fptr(djo), _lib.fptr(dbetas), _lib.fptr(dorient), _lib.fptr(dpose)),
                   "bf_smpl_vjp")
        return dbetas, dorient, dpose

    def _smplx_params(self, betas, global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose):
        if self.model_type != "smplx":
            raise _lib.BodyfitError("forward_smplx / vjp_smplx: SMPL-X-kind models only (bf_smplx_forward)")
        betas = _f32(betas, (-1, self.n_betas))
        n = betas.shape[0]
        opt = lambda a, w: None if a is None else _f32(a, (n, w))          # noqa: E731
        arrays = (betas, _f32(global_orient, (n, 3)), _f32(body_pose, (n, 63)), opt(jaw_pose, 3), opt(leye_pose, 3), opt(reye_pose, 3),
                  opt(left_hand_pose, self.n_hand_pca), opt(right_hand_pose, self.n_hand_pca))
        return n, arrays, _lib.SmplxParams(*[_lib.fptr(a) for a in arrays])

    def _expression(self, expression, n):
        if expression is None:
            return None
        if self.n_expression == 0:
            raise _lib.BodyfitError("expression: the model has no expression directions (bf_model_set_expression)")
        return _f32(expression, (n, self.n_expression))

    def forward_smplx(self, betas, global_orient, body_pose, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
                      right_hand_pose=None, expression=None):
        """smplx.create(model_type='smplx', ...).forward as smplify.py:177-190 calls it (bf_smplx_forward), model space; an
        argument left None is zeros.  expression[n,n_expression] (None: the call without it, bit for bit) goes through
        bf_smplx_forward_expr on a model with expression directions.  -> dict(vertices[n,NV,3], joints[n,n_joint_map,3] (the
        model's joint_map: 135), joints_all[n,144,3] (what smplx returns before a joint_mapper), full_pose[n,165], dyn_row[n] int32)."""
        n, keep, par = self._smplx_params(betas, global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose)
        expr = self._expression(expression, n)
        out = {"vertices": np.empty((n, self.n_verts, 3), np.float32), "joints": np.empty((n, self.n_joint_map, 3), np.float32),
               "joints_all": np.empty((n, self.n_joints_all, 3), np.float32), "full_pose": np.empty((n, 3 * self.n_joints), np.float32),
               "dyn_row": np.empty(n, np.int32)}
        dst = _lib.SmplxOutputs(*[_lib.fptr(out[k]) for k in ("vertices", "joints", "joints_all", "full_pose")], _lib.iptr(out["dyn_row"]))
        if expr is None:
            _lib.check(self._lib.bf_smplx_forward(self._h, n, C.byref(par), C.byref(dst)), "bf_smplx_forward")
        else:
            _lib.check(self._lib.bf_smplx_forward_expr(self._h, n, C.byref(par), _lib.fptr(expr), C.byref(dst)), "bf_smplx_forward_expr")
        return out

    def vjp_smplx(self, betas, global_orient, body_pose, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
                  right_hand_pose=None, dverts=None, djoints=None, djoints_all=None, dfull_pose=None, expression=None, want_dexpression=True):
        """The backward of `forward_smplx` (bf_smplx_vjp): cotangents of vertices, joints, joints_all, full_pose (None = zero) ->
        (dbetas, dglobal_orient, dbody_pose, djaw_pose, dleye_pose, dreye_pose, dleft_hand_pose, dright_hand_pose), each [n, .].
        With expression[n,n_expression] (bf_smplx_vjp_expr) a ninth entry follows: dexpression[n,n_expression], or None with
        want_dexpression=False - the other eight are then the same bits.
        No gradient flows through the contour landmarks' row choice."""
        n, keep, par = self._smplx_params(betas, global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose)
        expr = self._expression(expression, n)
        shapes = ((n, self.n_verts, 3), (n, self.n_joint_map, 3), (n, self.n_joints_all, 3), (n, 3 * self.n_joints))
        cots = [None if a is None else _f32(a, sh) for a, sh in zip((dverts, djoints, djoints_all, dfull_pose), shapes)]
        widths = (self.n_betas, 3, 63, 3, 3, 3, self.n_hand_pca, self.n_hand_pca)
        grads = tuple(np.empty((n, w), np.float32) for w in widths)
        cot = _lib.SmplxCotangents(*[_lib.fptr(a) for a in cots])
        dst = _lib.SmplxGrads(*[_lib.fptr(g) for g in grads])
        if expr is None:
            _lib.check(self._lib.bf_smplx_vjp(self._h, n, C.byref(par), C.byref(cot), C.byref(dst)), "bf_smplx_vjp")
            return grads
        dexpr = np.empty((n, self.n_expression), np.float32) if want_dexpression else None
        _lib.check(self._lib.bf_smplx_vjp_expr(self._h, n, C.byref(par), _lib.fptr(expr), C.byref(cot), C.byref(dst), _lib.fptr(dexpr)),
                   "bf_smplx_vjp_expr")
        return grads + (dexpr,)

    def forward_packed(self, params):
        """vertices / joints (model space) of packed parameter vectors [n, n_params] - any model kind"""
        p = _f32(params, (-1, self.n_params))
        verts = np.empty((len(p), self.n_verts, 3), np.float32)
        joints = np.empty((len(p), self.n_joint_map, 3), np.float32)
        _lib.check(self._lib.bf_model_forward(self._h, len(p), _lib.fptr(p), _lib.fptr(verts), _lib.fptr(joints)), "bf_model_forward")
        return verts, joints


class Scan:
    """A scan mesh with its closest-point grid on the GPU (reference utils/mesh_grid_searcher.py:51-84)."""

    def __init__(self, verts, faces, device=0):
        self._lib = _lib.load()
        v = _f32(verts, (-1, 3))
        f = _i32(np.asarray(faces).reshape(-1, 3))
        self.n_verts, self.n_faces, self.device = len(v), len(f), int(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_scan_create(int(device), len(v), _lib.fptr(v), len(f), _lib.iptr(f), C.byref(self._h)),
                   "bf_scan_create")
        self.height = float(self._lib.bf_scan_height(self._h))
        self.dev_route_device = self.device if offers_mesh_loss_dev(self._lib) else None       # the GPU a device route is offered on

    def close(self):
        _close_workspace(self)
        if getattr(self, "_h", None):
            self._lib.bf_scan_destroy(self._h)
            self._h = None

    def workspace(self):
        """the scan's own `Workspace` for the device route, made on first use and closed with the scan"""
        return _own_workspace(self)

    # The device route: the calls below take device ADDRESSES (integers; 0 / None = NULL) of contiguous arrays on the scan's GPU and
    # queue their work on `stream` (a hipStream_t handle); nothing is read back.

    def point_loss_dev(self, n, stream, points, loss=0, face_ids=0, nearest=0, dpoints=0, ws=None):
        """`point_loss` (bf_scan_point_loss_dev): points[n,3] -> loss[1], face_ids[n] int32, nearest[n,3], dpoints[n,3]"""
        ws = ws or self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_scan_point_loss_dev(self._h, int(n), points or None, loss or None, face_ids or None, nearest or None,
                                                        dpoints or None, ws._h, stream or None), "bf_scan_point_loss_dev")

    def nearest_points_dev(self, n, stream, points, face_ids=0, nearest=0, bary=0, ws=None):
        """`nearest_points` (bf_scan_nearest_dev): points[n,3] -> face_ids[n] int32, nearest[n,3], bary[n,3]"""
        ws = ws or self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_scan_nearest_dev(self._h, int(n), points or None, face_ids or None, nearest or None, bary or None,
                                                     ws._h, stream or None), "bf_scan_nearest_dev")

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def grid_info(self):
        dims = np.zeros(3, np.int32)
        os_ = np.zeros(4, np.float32)
        _lib.check(self._lib.bf_scan_grid_info(self._h, _lib.iptr(dims), _lib.fptr(os_)), "bf_scan_grid_info")
        return dims, os_[:3], float(os_[3])

    def grid_lists(self):
        """-> (tri_num int32[cells] inclusive cumsum, tri_idx int32[entries] face id + 1): insert_grid_surface's outputs"""
        dims, _, _ = self.grid_info()
        n = np.zeros(1, np.int32)
        _lib.check(self._lib.bf_scan_grid_lists(self._h, None, None, _lib.iptr(n)), "bf_scan_grid_lists")
        tri_num = np.empty(int(np.prod(dims)), np.int32)
        tri_idx = np.empty(max(int(n[0]), 1), np.int32)
        _lib.check(self._lib.bf_scan_grid_lists(self._h, _lib.iptr(tri_num), _lib.iptr(tri_idx), None), "bf_scan_grid_lists")
        return tri_num, tri_idx[:int(n[0])]

    def inside_mesh(self, points):
        """-> float32[n]: +1 inside the scan surface, -1 outside (MeshGridSearcher.inside_mesh)"""
        p = _f32(points, (-1, 3))
        sign = np.empty(len(p), np.float32)
        _lib.check(self._lib.bf_scan_inside(self._h, len(p), _lib.fptr(p), _lib.fptr(sign)), "bf_scan_inside")
        return sign

    def intersects_any(self, origins, directions):
        """-> bool[n]: does the ray origin + t direction (t >= 0) hit the scan surface (MeshGridSearcher.intersects_any)"""
        o = _f32(origins, (-1, 3))
        d = _f32(directions, (len(o), 3))
        hit = np.empty(len(o), np.uint8)
        _lib.check(self._lib.bf_scan_intersects(self._h, len(o), _lib.fptr(o), _lib.fptr(d), hit.ctypes.data_as(C.POINTER(C.c_uint8))),
                   "bf_scan_intersects")
        return hit.astype(bool)

    def nearest_points(self, points):
        """-> (nearest points [n,3], face ids [n], barycentrics [n,3]) like MeshGridSearcher.nearest_points"""
        p = _f32(points, (-1, 3))
        ids = np.empty(len(p), np.int32)
        pts = np.empty((len(p), 3), np.float32)
        bary = np.empty((len(p), 3), np.float32)
        _lib.check(self._lib.bf_scan_nearest(self._h, len(p), _lib.fptr(p), _lib.iptr(ids), _lib.fptr(pts), _lib.fptr(bary)),
                   "bf_scan_nearest")
        return pts, ids, bary

    def nearest_points_hinted(self, points, hint=None, reps=0):
        """nearest_points with a guess per query (hint[n,3]: e.g. the previous iteration's nearest points; any values are safe - the
        kernel checks the guess).  -> (points, ids, barycentrics[, mean kernel microseconds when reps > 0])"""
        p = _f32(points, (-1, 3))
        h = None if hint is None else _f32(hint, (len(p), 3))
        ids = np.empty(len(p), np.int32)
        pts = np.empty((len(p), 3), np.float32)
        bary = np.empty((len(p), 3), np.float32)
        us = C.c_float(0.0)
        _lib.check(self._lib.bf_scan_nearest_hinted(self._h, len(p), _lib.fptr(p), _lib.fptr(h), _lib.iptr(ids), _lib.fptr(pts), _lib.fptr(bary),
                                                    int(reps), C.byref(us)), "bf_scan_nearest_hinted")
        return (pts, ids, bary, us.value) if reps > 0 else (pts, ids, bary)


    def point_loss(self, points, want_grad=True):
        """bf_scan_point_loss: point_cloud_loss_mesh_grid (loss.py:233-242) of points[n,3] in one call - the search, then the
        reduction on the points already uploaded.  -> (loss float32 scalar, face ids [n], nearest points [n,3], dpoints [n,3] =
        the gradient for cotangent 1, exactly zero where the loss is zero; None unless want_grad)"""
        p = _f32(points, (-1, 3))
        loss = np.empty(1, np.float32)
        ids = np.empty(len(p), np.int32)
        pts = np.empty((len(p), 3), np.float32)
        dp = np.empty((len(p), 3), np.float32) if want_grad else None
        _lib.check(self._lib.bf_scan_point_loss(self._h, len(p), _lib.fptr(p), _lib.fptr(loss), _lib.iptr(ids), _lib.fptr(pts), _lib.fptr(dp)),
                   "bf_scan_point_loss")
        return loss[0], ids, pts, dp

    def nearest_points_backward(self, face_ids, bary, dnearest):
        """dL/d(query points) from dL/d(nearest points): SurfaceNearest.backward w.r.t. its first argument (point-to-plane
        where the closest point lies on a face, along the edge on an edge, zero at a corner)"""
        ids = _i32(face_ids)
        b = _f32(bary, (len(ids), 3))
        g = _f32(dnearest, (len(ids), 3))
        out = np.empty((len(ids), 3), np.float32)
        _lib.check(self._lib.bf_scan_nearest_backward(self._h, len(ids), _lib.iptr(ids), _lib.fptr(b), _lib.fptr(g), _lib.fptr(out)),
                   "bf_scan_nearest_backward")
        return out


class Topology:
    """A mesh's faces[NF,3] and its vertex -> (face, corner) lists uploaded once to one GPU (bf_topo): what compute_normal_torch
    and normal_laplacian_smoothness walk."""

    def __init__(self, n_verts, faces, device=0):
        lib = _lib.load()
        self._lib = lib
        f = _i32(np.asarray(faces).reshape(-1, 3))
        self.n_verts, self.n_faces, self.device = int(n_verts), len(f), int(device)
        self._h = C.c_void_p()
        _lib.check(lib.bf_topo_create(self.device, self.n_verts, self.n_faces, _lib.iptr(f), C.byref(self._h)), "bf_topo_create")
        self.dev_route_device = self.device if offers_mesh_loss_dev(lib) else None       # the GPU a device route is offered on

    def close(self):
        _close_workspace(self)
        if getattr(self, "_h", None):
            self._lib.bf_topo_destroy(self._h)
            self._h = None

    def workspace(self):
        """the topology's own `Workspace` for the device route - the normals, their reverse and the Laplacian share it - made on first
        use and closed with the topology"""
        return _own_workspace(self)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def vertex_normals(topo, verts):
    """bf_vertex_normals: compute_normal_torch (io_utils.py:406-428), verts[NV,3] -> normals[NV,3]"""
    v = _f32(verts, (topo.n_verts, 3))
    out = np.empty((topo.n_verts, 3), np.float32)
    _lib.check(topo._lib.bf_vertex_normals(topo._h, _lib.fptr(v), _lib.fptr(out)), "bf_vertex_normals")
    return out


def vertex_normals_vjp(topo, verts, dnormals):
    """bf_vertex_normals_vjp: dnormals[NV,3] (any cotangent of the normals) -> dverts[NV,3]"""
    v = _f32(verts, (topo.n_verts, 3))
    dn = _f32(dnormals, (topo.n_verts, 3))
    out = np.empty((topo.n_verts, 3), np.float32)
    _lib.check(topo._lib.bf_vertex_normals_vjp(topo._h, _lib.fptr(v), _lib.fptr(dn), _lib.fptr(out)), "bf_vertex_normals_vjp")
    return out


def normal_laplacian(topo, norms, want_grad=True):
    """bf_normal_laplacian: normal_laplacian_smoothness (loss.py:273-288) of norms[NV,3] -> (loss float32 scalar, dnorms[NV,3] =
    the gradient for cotangent 1; None unless want_grad)"""
    n = _f32(norms, (topo.n_verts, 3))
    loss = np.empty(1, np.float32)
    dn = np.empty((topo.n_verts, 3), np.float32) if want_grad else None
    _lib.check(topo._lib.bf_normal_laplacian(topo._h, _lib.fptr(n), _lib.fptr(loss), _lib.fptr(dn)), "bf_normal_laplacian")
    return loss[0], dn


def normal_loss(closest_face_norms, point_norms, want_grad=True, device=0):
    """bf_normal_loss: normal_loss_mesh_grid (loss.py:260-271) behind the search, closest_face_norms[n,3] = face_norm_mesh[closest
    face] -> (loss float32 scalar, dpoint_norms[n,3] = the gradient for cotangent 1; None unless want_grad)"""
    fn = _f32(closest_face_norms, (-1, 3))
    pn = _f32(point_norms, (len(fn), 3))
    loss = np.empty(1, np.float32)
    dpn = np.empty((len(fn), 3), np.float32) if want_grad else None
    _lib.check(_lib.load().bf_normal_loss(int(device), len(fn), _lib.fptr(fn), _lib.fptr(pn), _lib.fptr(loss), _lib.fptr(dpn)), "bf_normal_loss")
    return loss[0], dpn


# The device route of the five calls above: device ADDRESSES (integers; 0 / None = NULL) of contiguous float32 arrays on the topology's /
# the given GPU, queued on `stream` (a hipStream_t handle); nothing is read back.  ws: a `Workspace` (None: the topology's own).

def vertex_normals_dev(topo, stream, verts, normals, ws=None):
    """bf_vertex_normals_dev: verts[NV,3] -> normals[NV,3]"""
    ws = ws or topo.workspace()
    with ws.lock:
        _lib.check(topo._lib.bf_vertex_normals_dev(topo._h, verts or None, normals or None, ws._h, stream or None), "bf_vertex_normals_dev")


def vertex_normals_vjp_dev(topo, stream, verts, dnormals, dverts, ws=None):
    """bf_vertex_normals_vjp_dev: dnormals[NV,3] -> dverts[NV,3]"""
    ws = ws or topo.workspace()
    with ws.lock:
        _lib.check(topo._lib.bf_vertex_normals_vjp_dev(topo._h, verts or None, dnormals or None, dverts or None, ws._h, stream or None),
                   "bf_vertex_normals_vjp_dev")


def normal_laplacian_dev(topo, stream, norms, loss=0, dnorms=0, ws=None):
    """bf_normal_laplacian_dev: norms[NV,3] -> loss[1], dnorms[NV,3] (the gradient for cotangent 1)"""
    ws = ws or topo.workspace()
    with ws.lock:
        _lib.check(topo._lib.bf_normal_laplacian_dev(topo._h, norms or None, loss or None, dnorms or None, ws._h, stream or None),
                   "bf_normal_laplacian_dev")


def normal_loss_dev(ws, stream, n, face_ids, face_norm_table, n_faces, point_norms, loss=0, dpoint_norms=0):
    """bf_normal_loss_dev on the workspace's GPU: face_ids[n] int32 and the whole face_norm_table[n_faces,3], gathered in the kernel"""
    with ws.lock:
        _lib.check(_lib.load().bf_normal_loss_dev(ws.device, int(n), face_ids or None, face_norm_table or None, int(n_faces),
                                                  point_norms or None, loss or None, dpoint_norms or None, ws._h, stream or None),
                   "bf_normal_loss_dev")


def scale_gradient_dev(device, stream, n, grad, cotangent, out, plus_zero=False):
    """bf_scale_gradient_dev: out[n] = grad[n] * cotangent[0] (+ 0.0 with plus_zero), the cotangent read on the device"""
    _lib.check(_lib.load().bf_scale_gradient_dev(int(device), int(n), grad or None, cotangent or None, int(bool(plus_zero)), out or None,
                                                 stream or None), "bf_scale_gradient_dev")


# the device route of the silhouette term (bf_silhouette_*_dev of csrc/silhouette_api.hip)
SILHOUETTE_DEV_SYMBOLS = ("bf_silhouette_create_dev", "bf_silhouette_contours_dev", "bf_silhouette_loss_dev", "bf_scale_gradient_dev")
MASK_UINT8, MASK_FLOAT32 = 0, 1
SIL_EMPTY_VIEW = 1


def silhouette_rows_dev(device, stream, n_views, w2c, K, rows):
    """bf_silhouette_rows_dev: device addresses of w2c[M,4,4], K[M,3,3] -> rows[M,3,4] = K [R|t], the first launch of
    bf_silhouette_loss_dev by itself"""
    _lib.check(_lib.load().bf_silhouette_rows_dev(int(device), int(n_views), w2c or None, K or None, rows or None, stream or None),
               "bf_silhouette_rows_dev")


class MasksRefused(ValueError):
    """bf_silhouette_create_dev found, on the device, masks it does not take: `view` None = a value other than 0 / 1, else the
    first view with no foreground"""

    def __init__(self, view):
        super().__init__("masks hold a value other than 0 / 1" if view is None else f"mask {view} has no foreground")
        self.view = view


class Silhouette:
    """The masks[M,H,W] (truthy = foreground) of M views and one contour per view, kept on one GPU (bf_silhouette): what
    multview_mask_loss (loss.py:85-130) compares a caller's vertices with.  contours: None = the external borders are followed on
    the device and the one `contour_select` names is kept, else M arrays [C,2] (or [C,1,2]) of (x, y) points.
    `from_device` builds one from masks that are on the GPU already; `contours_dev` / `loss_dev` are the device route of `contours`
    / `loss` on any Silhouette (device addresses in, nothing read back), on the object's own `Workspace`."""

    @classmethod
    def offers_dev(cls, lib=None):
        """does the library export the silhouette's device route?"""
        lib = lib or _lib.load()
        return all(hasattr(lib, name) for name in SILHOUETTE_DEV_SYMBOLS)

    @classmethod
    def from_device(cls, masks, shape, mask_dtype, stream, device=0, contour_select=_lib.CONTOUR_OPENCV_FIRST):
        """bf_silhouette_create_dev: masks = the device address of shape = (M, H, W) contiguous elements of MASK_UINT8 (uint8, bool)
        or MASK_FLOAT32 on GPU `device`, possibly still in flight on `stream`.  Raises MasksRefused for a value other than 0 / 1 or
        a view without foreground; the pixels never reach the host"""
        self = cls.__new__(cls)
        self._lib = lib = _lib.load()
        self.n_views, self.H, self.W = (int(x) for x in shape)
        self.device = int(device)
        self._h = C.c_void_p()
        rc = lib.bf_silhouette_create_dev(self.device, self.n_views, self.H, self.W, masks or None, int(mask_dtype), int(contour_select),
                                          stream or None, C.byref(self._h))
        if rc >= SIL_EMPTY_VIEW:
            raise MasksRefused(rc - SIL_EMPTY_VIEW)
        if rc == -1 and b"0 / 1 only" in lib.bf_last_error():
            raise MasksRefused(None)
        _lib.check(rc, "bf_silhouette_create_dev")
        self.dev_route_device = self.device
        return self

    def __init__(self, masks, contours=None, device=0, contour_select=_lib.CONTOUR_OPENCV_FIRST):
        lib = _lib.load()
        self._lib = lib
        m = np.ascontiguousarray(np.asarray(masks) != 0, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        self.n_views, self.H, self.W = m.shape
        self.device = int(device)
        counts = xy = None
        if contours is not None:
            pts = [_f32(c, (-1, 2)) for c in contours]
            if len(pts) != self.n_views:
                raise ValueError(f"Silhouette: {len(pts)} contours for {self.n_views} masks")
            counts = np.array([len(p) for p in pts], np.int32)
            xy = np.ascontiguousarray(np.concatenate(pts + [np.zeros((1, 2), np.float32)]))
        self._h = C.c_void_p()
        _lib.check(lib.bf_silhouette_create(self.device, self.n_views, self.H, self.W, m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            _lib.iptr(counts), _lib.fptr(xy), int(contour_select), C.byref(self._h)), "bf_silhouette_create")
        self.dev_route_device = self.device if self.offers_dev(lib) else None       # the GPU a device route is offered on

    def workspace(self):
        """the object's own `Workspace` for the device route, made on first use and closed before the object"""
        return _own_workspace(self)

    def counts(self):
        """-> int32[M]: the contours' lengths (host values the object holds: no device work)"""
        counts = np.zeros(self.n_views, np.int32)
        _lib.check(self._lib.bf_silhouette_contours(self._h, _lib.iptr(counts), None), "bf_silhouette_contours")
        return counts

    def contours_dev(self, xy, stream):
        """bf_silhouette_contours_dev: the sum(counts()) (x, y) pairs copied device to device to the address `xy`, on `stream`"""
        _lib.check(self._lib.bf_silhouette_contours_dev(self._h, xy or None, stream or None), "bf_silhouette_contours_dev")

    def loss_dev(self, stream, n_verts, verts, w2c, K, imsize=512, epsilon=10, stride=4, cdist_form=True, terms=0, dverts=0, ws=None):
        """bf_silhouette_loss_dev: device addresses of verts[n_verts,3], w2c[M,4,4], K[M,3,3] -> terms[1 + 2M] (the loss, then per view
        (contour term, binary term)) and dverts[n_verts,3] (0 = not wanted), queued on `stream`; nothing is read back"""
        ws = ws or self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_silhouette_loss_dev(self._h, int(n_verts), int(stride), verts or None, w2c or None, K or None, float(imsize),
                                                        float(epsilon), int(bool(cdist_form)), terms or None, dverts or None, ws._h,
                                                        stream or None), "bf_silhouette_loss_dev")

    def contours(self):
        """-> list of M float32[C,2] arrays of (x, y) points in border order (bf_silhouette_contours)"""
        counts = np.zeros(self.n_views, np.int32)
        _lib.check(self._lib.bf_silhouette_contours(self._h, _lib.iptr(counts), None), "bf_silhouette_contours")
        xy = np.zeros((max(int(counts.sum()), 1), 2), np.float32)
        _lib.check(self._lib.bf_silhouette_contours(self._h, _lib.iptr(counts), _lib.fptr(xy)), "bf_silhouette_contours")
        ends = np.cumsum(counts)
        return [xy[e - c:e].copy() for c, e in zip(counts, ends)]

    def loss(self, verts, w2c, K, imsize=512, epsilon=10, stride=4, cdist_form=True, want_grad=True):
        """bf_silhouette_loss on verts[N,3][::stride] with cameras w2c[M,4,4], K[M,3,3] -> (value float32 scalar, view_terms[M,2] =
        per view (contour term, binary term), dverts[N,3] = the gradient for cotangent 1; None unless want_grad).  cdist_form:
        distances as torch.cdist computes them in float32 (expanded form beyond 25 inside vertices of a view), else direct sums"""
        v = _f32(verts, (-1, 3))
        w = _f32(w2c, (self.n_views, 4, 4))
        k = _f32(K, (self.n_views, 3, 3))
        loss = np.empty(1, np.float32)
        terms = np.empty((self.n_views, 2), np.float32)
        dv = np.empty((len(v), 3), np.float32) if want_grad else None
        _lib.check(self._lib.bf_silhouette_loss(self._h, len(v), int(stride), _lib.fptr(v), _lib.fptr(w), _lib.fptr(k), float(imsize),
                                                float(epsilon), int(bool(cdist_form)), _lib.fptr(loss), _lib.fptr(terms), _lib.fptr(dv)),
                   "bf_silhouette_loss")
        return loss[0], terms, dv

    def close(self):
        _close_workspace(self)
        if getattr(self, "_h", None):
            self._lib.bf_silhouette_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


TAPE_TEXTURES, TAPE_GEOMETRY = 1, 2          # BF_NR_TAPE_*
# the device route of the renderer (csrc/nr_api.hip)
NR_DEV_SYMBOLS = ("bf_nr_render_dev", "bf_nr_tape_texture_grad_dev", "bf_nr_tape_vertex_grad_dev", "bf_nr_tape_layout", "bf_nr_route_stats")
NR_TAPE_SEGMENTS = ("view", "pix", "frec", "light", "verts", "pv", "rgbmap", "unlit")


def nr_tape_layout(supersize, nrec, nv, lit, flags, has_rgb, directional):
    """bf_nr_tape_layout -> dict(offsets, sizes: per NR_TAPE_SEGMENTS name, in floats; total): the float32 storage a tape of
    NrRenderer.render_dev borrows.  flags 0: a render without a tape"""
    out = (C.c_uint64 * 17)()
    _lib.check(_lib.load().bf_nr_tape_layout(int(supersize), int(nrec), int(nv), int(bool(lit)), int(flags), int(bool(has_rgb)),
                                             int(bool(directional)), out), "bf_nr_tape_layout")
    v = [int(x) for x in out]
    return dict(offsets=dict(zip(NR_TAPE_SEGMENTS, v[:8])), sizes=dict(zip(NR_TAPE_SEGMENTS, v[8:16])), total=v[16])


def nr_route_stats():
    """bf_nr_route_stats -> dict(renders, growths, bytes_back): device-route renders, tile lists they grew, bytes they read back"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load().bf_nr_route_stats(out), "bf_nr_route_stats")
    return dict(zip(("renders", "growths", "bytes_back"), (int(v) for v in out)))


class NrRenderer:
    """bf_nr: neural_renderer.Renderer's image size, planes, background and light on one GPU (renderer.py:12-63)"""

    def __init__(self, image_size, anti_aliasing=True, near=0.1, far=100.0, background=(0.0, 0.0, 0.0), device=0):
        self._lib = _lib.load()
        self.image_size, self.device = int(image_size), int(device)
        self.supersize, self.directional = self.image_size * (2 if anti_aliasing else 1), 0.5
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_nr_create(self.device, self.image_size, int(bool(anti_aliasing)), float(near), float(far),
                                          _lib.fptr(_f32(background, (3,))), C.byref(self._h)), "bf_nr_create")

    def set_light(self, ambient, directional, color_ambient, color_directional, direction):
        _lib.check(self._lib.bf_nr_set_light(self._h, float(ambient), float(directional), _lib.fptr(_f32(color_ambient, (3,))),
                                             _lib.fptr(_f32(color_directional, (3,))), _lib.fptr(_f32(direction, (3,)))), "bf_nr_set_light")
        self.directional = float(np.float32(directional))

    @classmethod
    def offers_dev(cls, lib=None):
        """does the library export the device route's entry points?  One without them: every render takes the host route"""
        lib = lib or _lib.load()
        return all(hasattr(lib, name) for name in NR_DEV_SYMBOLS)

    def workspace(self):
        return _own_workspace(self)

    def tape_floats(self, mesh, fill_back, lit, flags, has_rgb):
        """how many floats the storage of a tape of this render holds (flags 0: no tape, no storage: 0)"""
        if not flags:
            return 0
        nrec = (2 if fill_back else 1) * mesh.textures_shape[0]
        return nr_tape_layout(self.supersize, nrec, mesh.n_verts, lit, flags, has_rgb, self.directional != 0.0)["total"]

    def render_dev(self, mesh, stream, verts, textures=0, K=None, R=None, t=None, orig_size=1.0, fill_back=True, lightoff=False, ndc=False,
                   rgb=0, depth=0, alpha=0, flags=0, storage=0, storage_floats=0):
        """bf_nr_render_dev: verts / textures / rgb / depth / alpha / storage are device addresses (0: none); each of K, R, t is an
        array (taken by value) or a device address (an int: read where it lies).  flags 0: no tape -> None, else -> an NrTape that
        borrows `storage` (the caller keeps it alive)"""
        host, dev = [], []
        for x, shape in ((K, (3, 3)), (R, (3, 3)), (t, (3,))):
            by_address = isinstance(x, int)
            host.append(None if ndc or by_address else _f32(x, shape))
            dev.append(x if by_address and not ndc else None)
        cam = _lib.NrCameraDev(*dev)
        h = C.c_void_p()
        ws = self.workspace()
        with ws.lock:
            _lib.check(self._lib.bf_nr_render_dev(self._h, mesh._h, _lib.fptr(host[0]), _lib.fptr(host[1]), _lib.fptr(host[2]), float(orig_size),
                                                  int(bool(fill_back)), int(bool(lightoff)), int(bool(ndc)), rgb or None, depth or None, alpha or None,
                                                  int(flags), C.byref(h) if flags else None, verts or None, textures or None, C.byref(cam),
                                                  storage or None, int(storage_floats), ws._h, stream or None), "bf_nr_render_dev")
        return NrTape(h, mesh.textures_shape, mesh.n_verts, self.image_size, workspace=ws) if flags else None

    def render(self, mesh, K=None, R=None, t=None, orig_size=1.0, fill_back=True, lightoff=False, ndc=False, want=("rgb", "depth", "alpha"),
               tape=False):
        """bf_nr_render -> (rgb[3,is,is] | None, depth[is,is] | None, alpha[is,is] | None, NrTape | None): the outputs named in `want`"""
        n = self.image_size
        rgb = np.empty((3, n, n), np.float32) if "rgb" in want else None
        depth = np.empty((n, n), np.float32) if "depth" in want else None
        alpha = np.empty((n, n), np.float32) if "alpha" in want else None
        cam = [None, None, None] if ndc else [_f32(K, (3, 3)), _f32(R, (3, 3)), _f32(t, (3,))]
        h = C.c_void_p()
        _lib.check(self._lib.bf_nr_render(self._h, mesh._h, _lib.fptr(cam[0]), _lib.fptr(cam[1]), _lib.fptr(cam[2]), float(orig_size),
                                          int(bool(fill_back)), int(bool(lightoff)), int(bool(ndc)), _lib.fptr(rgb), _lib.fptr(depth),
                                          _lib.fptr(alpha), C.byref(h) if tape else None), "bf_nr_render")
        return rgb, depth, alpha, (NrTape(h, mesh.textures_shape) if tape else None)

    def render_taped(self, mesh, K=None, R=None, t=None, orig_size=1.0, fill_back=True, lightoff=False, ndc=False, want=("rgb", "depth", "alpha"),
                     flags=TAPE_GEOMETRY):
        """bf_nr_render_taped: `render` with a tape that keeps what `flags` (TAPE_TEXTURES | TAPE_GEOMETRY) names"""
        n = self.image_size
        rgb = np.empty((3, n, n), np.float32) if "rgb" in want else None
        depth = np.empty((n, n), np.float32) if "depth" in want else None
        alpha = np.empty((n, n), np.float32) if "alpha" in want else None
        cam = [None, None, None] if ndc else [_f32(K, (3, 3)), _f32(R, (3, 3)), _f32(t, (3,))]
        h = C.c_void_p()
        _lib.check(self._lib.bf_nr_render_taped(self._h, mesh._h, _lib.fptr(cam[0]), _lib.fptr(cam[1]), _lib.fptr(cam[2]), float(orig_size),
                                                int(bool(fill_back)), int(bool(lightoff)), int(bool(ndc)), _lib.fptr(rgb), _lib.fptr(depth),
                                                _lib.fptr(alpha), int(flags), C.byref(h)), "bf_nr_render_taped")
        return rgb, depth, alpha, NrTape(h, mesh.textures_shape, mesh.n_verts, n)

    def close(self):
        if getattr(self, "_h", None):
            _close_workspace(self)
            self._lib.bf_nr_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class NrMesh:
    """bf_nr_mesh: vertices[NV,3], faces[NF,3] and (optionally) textures[NF,ts,ts,ts,3] resident on the renderer's GPU"""

    def __init__(self, renderer, verts, faces, texture_size=0, textures=None):
        self._lib = _lib.load()
        v, f = _f32(verts, (-1, 3)), _i32(np.asarray(faces).reshape(-1, 3))
        ts = int(texture_size)
        self.textures_shape, self.n_verts = (len(f), ts, ts, ts, 3), len(v)
        tex = None if textures is None else _f32(textures, self.textures_shape)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_nr_mesh_create(renderer._h, len(v), _lib.fptr(v), len(f), _lib.iptr(f), ts, _lib.fptr(tex), C.byref(self._h)),
                   "bf_nr_mesh_create")

    def set_textures(self, textures):
        _lib.check(self._lib.bf_nr_mesh_set_textures(self._h, _lib.fptr(_f32(textures, self.textures_shape))), "bf_nr_mesh_set_textures")

    def set_vertices(self, verts):
        _lib.check(self._lib.bf_nr_mesh_set_vertices(self._h, _lib.fptr(_f32(verts, (self.n_verts, 3)))), "bf_nr_mesh_set_vertices")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bf_nr_mesh_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class NrTape:
    """bf_nr_tape: what the texture VJP and (a geometry tape) the vertex / camera VJP need of one render"""

    def __init__(self, handle, textures_shape, n_verts=0, image_size=0, workspace=None):
        self._lib, self._h, self.textures_shape = _lib.load(), handle, tuple(textures_shape)
        self.n_verts, self.image_size = int(n_verts), int(image_size)
        self._workspace = workspace          # a tape of render_dev: its renderer's

    def vertex_grad_dev(self, stream, grad_verts, grad_rgb=0, grad_depth=0, grad_alpha=0, grad_R=0, grad_t=0):
        """bf_nr_tape_vertex_grad_dev: device addresses all (0: a zero cotangent / a gradient not wanted); grad_verts[NV,3] is written"""
        if not self._h:
            raise _lib.BodyfitError("NrTape.vertex_grad_dev: the tape was closed")
        with self._workspace.lock:
            _lib.check(self._lib.bf_nr_tape_vertex_grad_dev(self._h, grad_rgb or None, grad_depth or None, grad_alpha or None, grad_verts or None,
                                                            grad_R or None, grad_t or None, self._workspace._h, stream or None),
                       "bf_nr_tape_vertex_grad_dev")

    def texture_grad_dev(self, stream, grad_rgb, grad_textures):
        """bf_nr_tape_texture_grad_dev: grad_rgb[3,is,is] -> grad_textures[NF,ts,ts,ts,3], device addresses"""
        if not self._h:
            raise _lib.BodyfitError("NrTape.texture_grad_dev: the tape was closed")
        with self._workspace.lock:
            _lib.check(self._lib.bf_nr_tape_texture_grad_dev(self._h, grad_rgb or None, grad_textures or None, self._workspace._h, stream or None),
                       "bf_nr_tape_texture_grad_dev")

    def vertex_grad(self, grad_rgb=None, grad_depth=None, grad_alpha=None, camera=True):
        """cotangents in the outputs' shapes (None: zero) -> (d / d vertices [NV,3], d / d R [3,3], d / d t [3]); camera=False (an
        ndc render has none): the last two are None (bf_nr_tape_vertex_grad)"""
        if not self._h:
            raise _lib.BodyfitError("NrTape.vertex_grad: the tape was closed")
        n = self.image_size
        g = [None if x is None else _f32(x, shape) for x, shape in ((grad_rgb, (3, n, n)), (grad_depth, (n, n)), (grad_alpha, (n, n)))]
        gv = np.empty((self.n_verts, 3), np.float32)
        gR, gt = (np.empty((3, 3), np.float32), np.empty(3, np.float32)) if camera else (None, None)
        _lib.check(self._lib.bf_nr_tape_vertex_grad(self._h, _lib.fptr(g[0]), _lib.fptr(g[1]), _lib.fptr(g[2]), _lib.fptr(gv), _lib.fptr(gR),
                                                    _lib.fptr(gt)), "bf_nr_tape_vertex_grad")
        return gv, gR, gt

    def texture_grad(self, grad_rgb):
        """grad_rgb[3,is,is] -> d / d textures [NF,ts,ts,ts,3] (bf_nr_tape_texture_grad)"""
        if not self._h:
            raise _lib.BodyfitError("NrTape.texture_grad: the tape was closed")
        g = np.ascontiguousarray(grad_rgb, dtype=np.float32)
        out = np.empty(self.textures_shape, np.float32)
        _lib.check(self._lib.bf_nr_tape_texture_grad(self._h, _lib.fptr(g), _lib.fptr(out)), "bf_nr_tape_texture_grad")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bf_nr_tape_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def set_nearest_rule(rule):
    """The arithmetic of every closest-point search of the process: "reference" (default: search_nearest_proj as the reference's
    source evaluates it in float32, mesh_grid_kernel.cu:12-109 + matrix.h) or "fast" (2 x 2 normal equations, v_rcp_f32).
    -> the rule that was active before."""
    names = {"reference": _lib.NEAREST_REFERENCE, "fast": _lib.NEAREST_FAST}
    lib = _lib.load()
    before = lib.bf_nearest_rule_get()
    if lib.bf_nearest_rule_set(names[rule] if isinstance(rule, str) else int(rule)) != 0:
        raise ValueError("unknown closest-point rule %r" % (rule,))
    return "fast" if before == _lib.NEAREST_FAST else "reference"


def set_mask_fold(mode):
    """How the silhouette loss's contour gradients reach dL/dvertices inside a fit: "sums" (default: fixed-point atomic sums by the
    contour scan, bodyfit.h BF_MASK_FOLD_SUMS) or "gather" (the ordered float32 walk of rounds 2-4).  -> the mode that was active."""
    names = {"sums": 0, "gather": 1}
    lib = _lib.load()
    before = lib.bf_mask_fold_get()
    if lib.bf_mask_fold_set(names[mode] if isinstance(mode, str) else int(mode)) != 0:
        raise ValueError("unknown mask fold mode %r" % (mode,))
    return "gather" if before == 1 else "sums"


def make_hyper(**kw):
    h = _lib.Hyper()
    _lib.load().bf_hyper_default(C.byref(h))
    for k, v in kw.items():
        if not hasattr(h, k):
            raise TypeError(f"unknown hyper-parameter {k!r}")
        setattr(h, k, float(v))
    return h


class Gmm:
    """MaxMixturePrior's buffers (means[M,D], precisions[M,D,D], nll_weights[M]) uploaded once to one GPU (bf_gmm)."""

    def __init__(self, means, precisions, nll_weights, device=0):
        lib = _lib.load()
        self._lib = lib
        means = _f32(means)
        self.n_components, self.dim = means.shape
        prec = _f32(precisions, (self.n_components, self.dim, self.dim))
        nllw = _f32(nll_weights, (self.n_components,))
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.check(lib.bf_gmm_create(self.device, self.n_components, self.dim, _lib.fptr(means), _lib.fptr(prec), _lib.fptr(nllw),
                                     C.byref(self._h)), "bf_gmm_create")

    def close(self):
        _close_workspace(self)
        if getattr(self, "_h", None):
            self._lib.bf_gmm_destroy(self._h)
            self._h = None

    def workspace(self):
        """the `Workspace` of device-route losses with this prior, made on first use and closed with it"""
        return _own_workspace(self)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


KP_LOSS_OUTPUTS = ("terms", "djoints", "dposes", "dbetas")


def keypoint_loss(joints, w2c=None, K=None, keypoints=None, present=None, divisor=None, poses=None, betas=None, gmm=None, hyper=None,
                  dterms=None, want=KP_LOSS_OUTPUTS, device=0):
    """bf_keypoint_loss: multiview_keypoint_loss (loss.py:139-230) of n independent problems and its vector-Jacobian product.
    joints[n,R,3] (None: no rows), w2c[n,V,4,4], K[n,V,3,3], keypoints[n,V,R,3], present[n,V] (None: all), divisor[n] - w2c None =
    no views; poses[n,pose_dim] / betas[n,NB] (None: that prior is off); gmm: a `Gmm` or None; hyper: make_hyper(...) or None;
    dterms[n,4] (None: ones).  -> dict over `want` (a subset of KP_LOSS_OUTPUTS): terms[n,4], djoints[n,R,3], dposes, dbetas."""
    unknown = set(want) - set(KP_LOSS_OUTPUTS)
    if unknown:
        raise TypeError(f"unknown output(s) {sorted(unknown)}")
    if ("dposes" in want and poses is None) or ("dbetas" in want and betas is None):
        raise ValueError("keypoint_loss: a gradient was asked for an input that was not passed")
    q = _lib.KeypointLossIn()
    keep = {}
    if joints is not None:
        keep["joints"] = _f32(joints)
        if keep["joints"].ndim != 3 or keep["joints"].shape[2] != 3:
            raise ValueError("joints must be [n, rows, 3]")
        n, rows = keep["joints"].shape[:2]
    else:
        first = poses if poses is not None else betas
        if first is None:
            raise ValueError("keypoint_loss needs joints, poses or betas")
        n, rows = np.asarray(first).reshape(-1, np.asarray(first).shape[-1]).shape[0], 0
    n_views = 0
    if w2c is not None:
        keep["w2c"] = _f32(w2c)
        n_views = keep["w2c"].shape[1] if keep["w2c"].ndim == 4 else -1
        keep["w2c"] = keep["w2c"].reshape(n, n_views, 4, 4)
        keep["K"] = _f32(K, (n, n_views, 3, 3))
        keep["keypoints"] = _f32(keypoints, (n, n_views, rows, 3))
        keep["divisor"] = _i32(divisor).reshape(n)
        if present is not None:
            keep["present"] = np.ascontiguousarray(np.asarray(present).reshape(n, n_views) != 0, dtype=np.uint8)
            q.present = keep["present"].ctypes.data_as(C.POINTER(C.c_uint8))
        q.w2c, q.K, q.keypoints, q.divisor = (_lib.fptr(keep["w2c"]), _lib.fptr(keep["K"]), _lib.fptr(keep["keypoints"]),
                                              _lib.iptr(keep["divisor"]))
    q.n, q.n_views, q.n_rows, q.joints = n, n_views, rows, _lib.fptr(keep.get("joints"))
    if poses is not None:
        keep["poses"] = _f32(poses)
        keep["poses"] = keep["poses"].reshape(n, keep["poses"].shape[-1])
        q.pose_dim, q.poses = keep["poses"].shape[1], _lib.fptr(keep["poses"])
    if betas is not None:
        keep["betas"] = _f32(betas)
        keep["betas"] = keep["betas"].reshape(n, keep["betas"].shape[-1])
        q.n_betas, q.betas = keep["betas"].shape[1], _lib.fptr(keep["betas"])
    if dterms is not None:
        keep["dterms"] = _f32(dterms, (n, 4))
    out = {}
    if "terms" in want:
        out["terms"] = np.empty((n, 4), np.float32)
    if "djoints" in want:
        out["djoints"] = np.zeros((n, rows, 3), np.float32)
    if "dposes" in want:
        out["dposes"] = np.empty((n, q.pose_dim), np.float32)
    if "dbetas" in want:
        out["dbetas"] = np.empty((n, q.n_betas), np.float32)
    if gmm is not None:
        device = gmm.device
    _lib.check(_lib.load().bf_keypoint_loss(int(device), gmm._h if gmm is not None else None, C.byref(q),
                                            C.byref(hyper) if hyper is not None else None, _lib.fptr(keep.get("dterms")),
                                            _lib.fptr(out.get("terms")), _lib.fptr(out.get("djoints")), _lib.fptr(out.get("dposes")),
                                            _lib.fptr(out.get("dbetas"))), "bf_keypoint_loss")
    return out


_LOSS_WORKSPACES = {}          # device -> the Workspace of device-route losses without a GMM


def loss_workspace(gmm=None, device=0):
    """the workspace a device-route keypoint loss runs on: the GMM's, or, without one, the one of `device`"""
    if gmm is not None:
        return gmm.workspace()
    if int(device) not in _LOSS_WORKSPACES:
        _LOSS_WORKSPACES[int(device)] = Workspace(device)
    return _LOSS_WORKSPACES[int(device)]


def keypoint_loss_dev(stream, n, rows=0, joints=0, n_views=0, w2c=0, K=0, keypoints=0, present=0, divisor=None, pose_dim=0, poses=0,
                      n_betas=0, betas=0, gmm=None, hyper=None, dterms=0, terms=0, djoints=0, dposes=0, dbetas=0, device=0, ws=None):
    """bf_keypoint_loss_dev: `keypoint_loss` on device addresses (integers; 0 = NULL), queued on `stream`.  joints[n,rows,3],
    w2c[n,V,4,4], K[n,V,3,3], keypoints[n,V,rows,3], present[n,V] uint8, poses[n,pose_dim], betas[n,n_betas], dterms[n,4] ->
    terms[n,4], djoints, dposes, dbetas (0: not wanted).  divisor stays a host array of n ints.  ws: None = loss_workspace(gmm, device)."""
    ws = ws or loss_workspace(gmm, device)
    q = _lib.KeypointLossIn()
    q.n, q.n_views, q.n_rows, q.joints = int(n), int(n_views), int(rows), _lib.at(joints)
    keep = None
    if n_views:
        keep = _i32(divisor).reshape(n)
        q.w2c, q.K, q.keypoints, q.divisor = _lib.at(w2c), _lib.at(K), _lib.at(keypoints), _lib.iptr(keep)
        q.present = _lib.at(present, C.POINTER(C.c_uint8))
    q.pose_dim, q.poses, q.n_betas, q.betas = int(pose_dim), _lib.at(poses), int(n_betas), _lib.at(betas)
    with ws.lock:
        _lib.check(_lib.load().bf_keypoint_loss_dev(ws._h, stream or None, gmm._h if gmm is not None else None, C.byref(q),
                                                    C.byref(hyper) if hyper is not None else None, dterms or None, terms or None,
                                                    djoints or None, dposes or None, dbetas or None), "bf_keypoint_loss_dev")
    del keep


class FrameBatch:
    """F independent frames x V views resident on the model's GPU."""

    def __init__(self, dev_model: DeviceModel, n_frames, n_views):
        self._lib = dev_model._lib
        self.model = dev_model
        self.F, self.V = int(n_frames), int(n_views)
        self._h = C.c_void_p()
        _lib.check(self._lib.bf_batch_create(dev_model._h, self.F, self.V, C.byref(self._h)), "bf_batch_create")
        self._n_kp = self.F * self.V * self.model.n_loss_joints * 3
        self._stage_by_address = _lib.by_address("bf_batch_stage_inputs")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bf_batch_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- inputs ------------------------------------------------------------------------------
    def set_cameras(self, c2ws, Ks):
        c2w = _f32(c2ws, (self.F, self.V, 4, 4))
        K = _f32(Ks, (self.F, self.V, 3, 3))
        _lib.check(self._lib.bf_batch_set_cameras(self._h, _lib.fptr(c2w), _lib.fptr(K)), "bf_batch_set_cameras")

    def set_keypoints(self, keypoints, n_use_frames=None):
        kp = _f32(keypoints, (self.F, self.V, self.model.n_loss_joints, 3))
        nd = None if n_use_frames is None else _i32(np.broadcast_to(np.asarray(n_use_frames), (self.F,)))
        _lib.check(self._lib.bf_batch_set_keypoints(self._h, _lib.fptr(kp), _lib.iptr(nd)), "bf_batch_set_keypoints")

    def set_init(self, init_betas, init_pose):
        b = _f32(init_betas, (self.F, self.model.n_core_betas))
        p = _f32(np.asarray(init_pose).reshape(self.F, -1)[:, :72], (self.F, 72))
        _lib.check(self._lib.bf_batch_set_init(self._h, _lib.fptr(b), _lib.fptr(p)), "bf_batch_set_init")

    def stage_inputs(self, keypoints, n_use_frames, init_betas, init_pose):
        """the NEXT frame's keypoints + initial estimate without waiting for the fit in flight (bf_batch_stage_inputs); the next
        fit() must carry FIT_RESET.  Arrays that already are C-contiguous float32 / int32 of the right size are passed as they are, by
        address (the frame loop's case: the call costs what the library does); everything else - lists, other dtypes, strided views, a
        scalar n_use_frames, poses wider than 72 - is converted first."""
        at = stage_addresses(self.F, self._n_kp, self.model.n_core_betas, keypoints, n_use_frames, init_betas, init_pose)
        if at is not None:
            _lib.check(self._stage_by_address(self._h, at[0], at[1], at[2], at[3]), "bf_batch_stage_inputs")
            return
        kp = _f32(keypoints, (self.F, self.V, self.model.n_loss_joints, 3))
        nd = None if n_use_frames is None else _i32(np.broadcast_to(np.asarray(n_use_frames), (self.F,)))
        b = _f32(init_betas, (self.F, self.model.n_core_betas))
        p = _f32(np.asarray(init_pose).reshape(self.F, -1)[:, :72], (self.F, 72))
        _lib.check(self._lib.bf_batch_stage_inputs(self._h, _lib.fptr(kp), _lib.iptr(nd), _lib.fptr(b), _lib.fptr(p)), "bf_batch_stage_inputs")

    def set_scans(self, scans):
        """one Scan per frame (use_mesh=True); None detaches"""
        if scans is None:
            _lib.check(self._lib.bf_batch_set_scans(self._h, None), "bf_batch_set_scans")
            self._scans = None
            return
        assert len(scans) == self.F
        arr = (C.c_void_p * self.F)(*[s._h for s in scans])
        _lib.check(self._lib.bf_batch_set_scans(self._h, arr), "bf_batch_set_scans")
        self._scans = list(scans)          # keep them alive

    def set_masks(self, masks, view_index, contours=None, contour_select=_lib.CONTOUR_OPENCV_FIRST):
        """masks uint8[F,M,H,W] as loaded; view_index[M]; contours: F lists of M arrays [C,2] (x, y), or None to have them
        extracted from the masks on the device (use_mask=True, smplify.py:138-144); contour_select: which external border of a
        mask with several components is kept then (include/bodyfit.h, BF_CONTOUR_*)"""
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        F, M, H, W = masks.shape
        assert F == self.F
        vi = _i32(view_index)
        mp = masks.ctypes.data_as(C.POINTER(C.c_uint8))
        if contours is None:
            _lib.check(self._lib.bf_batch_set_masks(self._h, M, _lib.iptr(vi), H, W, mp, None, None, int(contour_select)), "bf_batch_set_masks")
            return
        counts = _i32([[len(c) for c in per_frame] for per_frame in contours]).reshape(-1)
        flat = [np.asarray(c, np.float32).reshape(-1, 2) for per_frame in contours for c in per_frame]
        xy = _f32(np.concatenate(flat, 0)) if sum(len(c) for c in flat) else np.zeros((1, 2), np.float32)
        _lib.check(self._lib.bf_batch_set_masks(self._h, M, _lib.iptr(vi), H, W, mp, _lib.iptr(counts), _lib.fptr(xy), 0), "bf_batch_set_masks")

    def stage_masks(self, masks, view_index, contour_select=_lib.CONTOUR_OPENCV_FIRST):
        """the NEXT frame's masks (same views and shape as the ones attached with set_masks(contours=None)): uploaded and
        border-followed under the fit in flight, used by the next fit()"""
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        F, M, H, W = masks.shape
        assert F == self.F
        vi = _i32(view_index)
        _lib.check(self._lib.bf_batch_stage_masks(self._h, M, _lib.iptr(vi), H, W, masks.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  int(contour_select)), "bf_batch_stage_masks")

    def clear_masks(self):
        """detach the silhouettes (use_mask=False for the next fit)"""
        _lib.check(self._lib.bf_batch_set_masks(self._h, 0, None, 0, 0, None, None, None, 0), "bf_batch_set_masks")

    def mask_loss(self, hyper=None):
        loss = np.empty(self.F, np.float32)
        dv = np.empty((self.F, self.model.n_verts, 3), np.float32)
        hp = C.byref(hyper) if hyper is not None else None
        _lib.check(self._lib.bf_batch_mask_loss(self._h, hp, _lib.fptr(loss), _lib.fptr(dv)), "bf_batch_mask_loss")
        return loss, dv

    def fit_displacement(self, n_iters, hyper=None):
        """SMPL+D stage (smplify.py:228-247) on the vertices of the last fit"""
        hp = C.byref(hyper) if hyper is not None else None
        _lib.check(self._lib.bf_fit_displacement(self._h, int(n_iters), hp), "bf_fit_displacement")

    def get_displacement(self):
        d = np.empty((self.F, self.model.n_verts, 3), np.float32)
        _lib.check(self._lib.bf_batch_get_displacement(self._h, _lib.fptr(d)), "bf_batch_get_displacement")
        return d

    def reset(self):
        """re-arm for another fit of the same inputs (stream-ordered, no host traffic)"""
        _lib.check(self._lib.bf_batch_reset(self._h), "bf_batch_reset")

    def set_params(self, params):
        p = _f32(params, (self.F, self.model.n_params))
        _lib.check(self._lib.bf_batch_set_params(self._h, _lib.fptr(p)), "bf_batch_set_params")

    # -- compute -----------------------------------------------------------------------------
    def fit(self, n_iters, hyper=None, flags=_lib.FIT_DEFAULT):
        hp = C.byref(hyper) if hyper is not None else None
        _lib.check(self._lib.bf_fit(self._h, int(n_iters), hp, int(flags)), "bf_fit")

    def sync(self):
        _lib.check(self._lib.bf_batch_sync(self._h), "bf_batch_sync")

    def loss_grad(self, hyper=None):
        terms = np.empty((self.F, 4), np.float32)
        grads = np.empty((self.F, self.model.n_params), np.float32)
        hp = C.byref(hyper) if hyper is not None else None
        _lib.check(self._lib.bf_loss_grad(self._h, hp, _lib.fptr(terms), _lib.fptr(grads)), "bf_loss_grad")
        return terms, grads

    def dense_iter_grad(self, hyper=None, late=False, sub_model=False, dverts_extra=None):
        """(terms[F,6], grads[F,n_params]) of one dense iteration of fit() at the current parameters, without the step
        (bf_dense_iter_grad); dverts_extra[F,NV,3]: a cotangent added onto dL/d(body vertices)"""
        terms = np.empty((self.F, 6), np.float32)
        grads = np.empty((self.F, self.model.n_params), np.float32)
        hp = C.byref(hyper) if hyper is not None else None
        extra = None if dverts_extra is None else _f32(dverts_extra, (self.F, self.model.n_verts, 3))
        flags = (_lib.DENSE_GRAD_LATE if late else 0) | (_lib.DENSE_GRAD_SUBMODEL if sub_model else 0)
        _lib.check(self._lib.bf_dense_iter_grad(self._h, hp, flags, _lib.fptr(extra), _lib.fptr(terms), _lib.fptr(grads)),
                   "bf_dense_iter_grad")
        return terms, grads

    # -- outputs -----------------------------------------------------------------------------
    def get_params(self):
        p = np.empty((self.F, self.model.n_params), np.float32)
        _lib.check(self._lib.bf_batch_get_params(self._h, _lib.fptr(p)), "bf_batch_get_params")
        return p

    def get_result(self, vertices=True):
        m = self.model
        verts = np.empty((self.F, m.n_verts, 3), np.float32) if vertices else None
        joints = np.empty((self.F, m.n_joint_map, 3), np.float32) if vertices else None
        full_pose = np.empty((self.F, 3 * m.n_joints), np.float32)
        terms = np.empty((self.F, 4), np.float32)
        _lib.check(self._lib.bf_batch_get_result(self._h, _lib.fptr(verts), _lib.fptr(joints), _lib.fptr(full_pose),
                                                 _lib.fptr(terms)), "bf_batch_get_result")
        return verts, joints, full_pose, terms

    def get_previous(self, vertices=True):
        """(params, vertices, joints, full_pose, terms) of the fit issued BEFORE the last one, while the last one runs
        (bf_batch_get_previous): the frame loop as a two-deep pipeline"""
        m = self.model
        params = np.empty((self.F, m.n_params), np.float32)
        verts = np.empty((self.F, m.n_verts, 3), np.float32) if vertices else None
        joints = np.empty((self.F, m.n_joint_map, 3), np.float32) if vertices else None
        full_pose = np.empty((self.F, 3 * m.n_joints), np.float32)
        terms = np.empty((self.F, 4), np.float32)
        _lib.check(self._lib.bf_batch_get_previous(self._h, _lib.fptr(params), _lib.fptr(verts), _lib.fptr(joints), _lib.fptr(full_pose),
                                                   _lib.fptr(terms)), "bf_batch_get_previous")
        return params, verts, joints, full_pose, terms

    def export_params_dev(self, dev_ptr):
        _lib.check(self._lib.bf_batch_export_params_dev(self._h, C.c_void_p(int(dev_ptr))), "bf_batch_export_params_dev")

    def last_timing(self):
        ms = np.zeros(4, np.float32)
        _lib.check(self._lib.bf_batch_last_timing(self._h, _lib.fptr(ms)), "bf_batch_last_timing")
        return {"fit_ms": float(ms[0]), "mesh_ms": float(ms[1]), "tail_ms": float(ms[2]), "total_ms": float(ms[3])}

    def timing_reset(self):
        _lib.check(self._lib.bf_batch_timing_reset(self._h), "bf_batch_timing_reset")

    def timing_sum(self):
        ms = np.zeros(4, np.float32)
        n = C.c_int32(0)
        _lib.check(self._lib.bf_batch_timing_sum(self._h, _lib.fptr(ms), C.byref(n)), "bf_batch_timing_sum")
        return {"fit_ms": float(ms[0]), "mesh_ms": float(ms[1]), "tail_ms": float(ms[2]), "total_ms": float(ms[3]),
                "calls": int(n.value)}

    def mesh_span(self, reps=50):
        """the single-frame full-mesh forward's own duration, measured inside the kernel -> {"mean_us", "min_us", "max_us"}"""
        us = np.zeros(3, np.float32)
        _lib.check(self._lib.bf_batch_mesh_span(self._h, int(reps), _lib.fptr(us)), "bf_batch_mesh_span")
        return {"mean_us": float(us[0]), "min_us": float(us[1]), "max_us": float(us[2])}

    DENSE_CLASSES = ("state_and_forward_mesh", "keypoint_and_silhouette_losses", "closest_point_search", "point_cloud_loss_and_gradient",
                     "reverse_mesh", "partial_block_reduction")

    def dense_timing(self, enable=True, read=False):
        """device milliseconds of the kernel classes of the last dense iteration of the last fit (bf_batch_dense_timing)"""
        ms = np.zeros(6, np.float32) if read else None
        _lib.check(self._lib.bf_batch_dense_timing(self._h, int(bool(enable)), _lib.fptr(ms)), "bf_batch_dense_timing")
        return None if ms is None else dict(zip(self.DENSE_CLASSES, (float(x) for x in ms)))

    def dense_resident(self):
        """True / False: the last dense fit ran with the fit kernel resident / one launch per iteration; None: no dense fit yet"""
        r = self._lib.bf_batch_dense_resident(self._h)
        return None if r < 0 else bool(r)

    def debug_vertices(self):
        """the body vertices [F,NV,3] the last full-model mesh pass left on the device (bf_batch_debug_vertices)"""
        v = np.empty((self.F, self.model.n_verts, 3), np.float32)
        _lib.check(self._lib.bf_batch_debug_vertices(self._h, _lib.fptr(v)), "bf_batch_debug_vertices")
        return v

    def lane_stats(self):
        """fit-lane groups since the batch was created -> {"launches", "calls", "max_group", "width"} (bf_batch_lane_stats)"""
        out = np.zeros(4, np.int32)
        _lib.check(self._lib.bf_batch_lane_stats(self._h, _lib.iptr(out)), "bf_batch_lane_stats")
        return {"launches": int(out[0]), "calls": int(out[1]), "max_group": int(out[2]), "width": int(out[3])}

    def lane_feed_stats(self):
        """how the fit lanes were fed since the batch was created -> {"transfers", "host_copies", "device_copies", "waits"}
        (bf_batch_lane_feed_stats)"""
        out = np.zeros(4, np.int64)
        _lib.check(self._lib.bf_batch_lane_feed_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))), "bf_batch_lane_feed_stats")
        return {"transfers": int(out[0]), "host_copies": int(out[1]), "device_copies": int(out[2]), "waits": int(out[3])}

    def disp_moment(self):
        """first Adam moment [F,NV,3] of the SMPL+D displacement (bf_batch_debug_disp_moment)"""
        m = np.empty((self.F, self.model.n_verts, 3), np.float32)
        _lib.check(self._lib.bf_batch_debug_disp_moment(self._h, _lib.fptr(m)), "bf_batch_debug_disp_moment")
        return m

    def disp_moment2(self):
        """second Adam moment [F,NV,3] of the SMPL+D displacement (bf_batch_debug_disp_moment2)"""
        v = np.empty((self.F, self.model.n_verts, 3), np.float32)
        _lib.check(self._lib.bf_batch_debug_disp_moment2(self._h, _lib.fptr(v)), "bf_batch_debug_disp_moment2")
        return v

    def debug_dump(self, n):
        out = np.zeros(n, np.float32)
        _lib.check(self._lib.bf_batch_debug_dump(self._h, _lib.fptr(out), int(n)), "bf_batch_debug_dump")
        return out


SMPLX_EXTRA = (("leye_pose", 3), ("reye_pose", 3), ("left_hand_pose", 6), ("right_hand_pose", 6))


def split_params(packed, n_joints=24, n_betas=10):
    """packed[...,86] (SMPL) or [...,98] (SMPL-X) in optimiser order (reference smplify.py:167-173) -> named blocks."""
    p = np.asarray(packed)
    smplx = p.shape[-1] == 98
    nbp = 63 if smplx else 3 * (n_joints - 1)
    o = 4 + nbp + n_betas
    out = {"global_transl": p[..., 0:3], "scale": p[..., 3:4], "pose": p[..., 4:4 + nbp],
           "betas": p[..., 4 + nbp:o], "global_orient": p[..., o:o + 3]}
    if smplx:
        o += 3
        for name, n in SMPLX_EXTRA:
            out[name] = p[..., o:o + n]
            o += n
    return out


def pack_params(d):
    names = ("global_transl", "scale", "pose", "betas", "global_orient") + tuple(n for n, _ in SMPLX_EXTRA if n in d)
    return np.concatenate([np.asarray(d[k], dtype=np.float32).reshape(-1) for k in names]).astype(np.float32)


def pack_problem(problems):
    """list of synthetic.make_problem dicts -> (c2w[F,V,4,4], K[F,V,3,3], kp[F,V,25,3], ndiv[F], betas, pose)."""
    F, V = len(problems), len(problems[0]["c2ws"])
    c2w = np.stack([np.stack(p["c2ws"]) for p in problems]).astype(np.float32)
    K = np.stack([np.stack(p["Ks"]) for p in problems]).astype(np.float32)
    smplx = any(k is not None and "face" in k for k in problems[0]["keypoints"])
    kp = np.zeros((F, V, 135 if smplx else N_LOSS_JOINTS, 3), np.float32)
    for f, p in enumerate(problems):
        for v, k in enumerate(p["keypoints"]):
            if k is not None:                      # None view: confidence 0 everywhere (loss.py:157)
                kp[f, v] = pack_keypoints_smplx(k) if smplx else k["pose"]
    ndiv = np.array([len(p["use_frames"]) for p in problems], np.int32)
    betas = np.concatenate([p["init_betas"] for p in problems]).astype(np.float32)
    pose = np.concatenate([p["init_pose"] for p in problems]).astype(np.float32)
    return c2w, K, kp, ndiv, betas, pose
