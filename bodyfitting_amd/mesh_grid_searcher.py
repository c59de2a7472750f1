"""`utils.mesh_grid_searcher.MeshGridSearcher` of the reference (utils/mesh_grid_searcher.py:51-99; the same file sits in
thirdparty/mesh_grid/) over the HIP closest-point grid (`native.Scan`, the `bf_scan_*` entry points that replace the `mesh_grid`
pybind module, mesh_grid.cpp:129-136).

Same constructor and methods: `MeshGridSearcher(verts, faces)`, `set_mesh`, `nearest_points(points) -> (nearest points, face ids)`,
`inside_mesh(points) -> +1 / -1 per point`, `intersects_any(origins, directions) -> bool per ray`.  The attributes the reference
leaves on the instance after `set_mesh` are there too (`verts`, `faces`, `step`, `num`, `minmax`, `tri_num`, `tri_idx` - the
grid the device built, read back lazily).  numpy in -> numpy out; torch tensors in -> torch tensors out on the tensors' device
(torch is imported only in that case).  float32 tensors on the scan's GPU are searched where they lie, on torch's current stream
(bf_scan_nearest_dev, the device route of _autograd.py, on the searcher's own workspace): `nearest_points` then returns tensors that
never left the GPU.  `inside_mesh` and `intersects_any` go through host memory.
"""
from __future__ import annotations

import numpy as np

from . import _autograd
from .native import Scan


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "cpu")


def memo_hit(memo, points):
    """is `memo` - (points tensor, its _version when it was searched, ...) or None - the answer for `points`?  Only for the SAME
    tensor object at the same version: the memo holds the tensor by strong reference, so no later tensor can take its identity (or
    its address) while the memo lives.  Contents are never compared - that is a read-back - and a miss merely searches again."""
    return memo is not None and memo[0] is points and memo[1] == points._version


def _to_np(x, dtype):
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))


class MeshGridSearcher:
    def __init__(self, verts=None, faces=None, device=0):
        self._scan = None
        self._device = device
        if verts is not None and faces is not None:
            self.set_mesh(verts, faces, device)

    @staticmethod
    def _device_index(device):
        if isinstance(device, int):
            return device
        if isinstance(device, str):                       # 'cuda:0' (the reference's default argument)
            return int(device.split(":")[1]) if ":" in device else 0
        idx = getattr(device, "index", None)
        return 0 if idx is None else int(idx)

    def set_mesh(self, verts, faces, device=0):
        """utils/mesh_grid_searcher.py:56-79: cell edge = (bounding-box volume / n_verts)^(1/3), the grid centred on the box;
        `insert_grid_surface` = bf_scan_create's build (count, scan, fill: the lists equal the reference's as sets per cell)"""
        self.close()
        self.verts = _to_np(verts, np.float32).reshape(-1, 3)
        self.faces = _to_np(faces, np.int32).reshape(-1, 3)
        self._scan = Scan(self.verts, self.faces, device=self._device_index(device))
        self._mesh_wants_grad = any(getattr(a, "requires_grad", False) for a in (verts, faces))
        self._last_query = None
        self._last_query_dev = None
        dims, origin, step = self._scan.grid_info()
        self.step = np.float32(step)
        self.num = np.concatenate([dims, [int(np.prod(dims))]]).astype(np.int32)          # [nx, ny, nz, nx ny nz]
        self.minmax = np.concatenate([origin, self.verts.max(0)]).astype(np.float32)      # [grid origin | max corner]
        self._lists = None

    def _grid_lists(self):
        if self._lists is None:
            self._lists = self._scan.grid_lists()
        return self._lists

    @property
    def tri_num(self):
        return self._grid_lists()[0]

    @property
    def tri_idx(self):
        return self._grid_lists()[1]

    def close(self):
        if getattr(self, "_scan", None) is not None:
            self._scan.close()               # (its workspace first: queued searches end before the grid goes)
            self._scan = None
        self._last_query = None
        self._last_query_dev = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _remember_query(self, points, ids, nearest):
        """the scan losses of one iteration query the same points (smplify.py:239-240): the last query's answer is kept beside a
        copy of its points"""
        self._last_query = (np.array(points, copy=True), ids, nearest)

    def _query(self, points):
        """-> (face ids, nearest points) of points[n,3]: the last query's when these are its points, else a search"""
        last = getattr(self, "_last_query", None)
        if last is not None and np.array_equal(last[0], points):
            return last[1], last[2]
        pts, ids, _ = self._scan.nearest_points(points)
        self._remember_query(points, ids, pts)
        return ids, pts

    # the device route's memo: the caller's points TENSOR (held, so that `is` is sound), its _version, and the answer as tensors

    def _remember_query_dev(self, points, ids, nearest):
        self._last_query_dev = (points, points._version, ids, nearest)

    def _query_dev(self, points, stream):
        """-> face ids (an int32 tensor [n] on the scan's GPU) of the tensor `points`: the last device query's when `memo_hit`, else a
        search queued on `stream` (bf_scan_nearest_dev)"""
        last = getattr(self, "_last_query_dev", None)
        if memo_hit(last, points):
            return last[2]
        ids, nearest = self._search_dev(points, stream)[:2]
        self._remember_query_dev(points, ids, nearest)
        return ids

    def _search_dev(self, points, stream, with_coefficients=False):
        import torch
        p = points.detach().reshape(-1, 3).contiguous()
        n = p.shape[0]
        ids = torch.empty(n, dtype=torch.int32, device=p.device)
        nearest = torch.empty((n, 3), dtype=torch.float32, device=p.device)
        bary = torch.empty((n, 3), dtype=torch.float32, device=p.device) if with_coefficients else None
        self._scan.nearest_points_dev(n, stream, p.data_ptr(), face_ids=ids.data_ptr(), nearest=nearest.data_ptr(),
                                      bary=0 if bary is None else bary.data_ptr())
        return ids, nearest, bary

    def _takes_device_route(self, *tensors):
        """float32 tensors on the scan's GPU, the switch on, the runtimes shared"""
        return _autograd.takes_device_route(getattr(self._scan, "dev_route_device", None), *tensors)

    def _need_mesh(self):
        if self._scan is None:
            raise RuntimeError("MeshGridSearcher: set_mesh() first")

    @staticmethod
    def _back(like, *arrays):
        if not _is_tensor(like):
            return arrays
        import torch
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(like.device) for a in arrays)

    def nearest_points(self, points):
        """:81-84 -> (nearest_pts[n,3] float32, nearest_faces[n] int32); no gradient, like the reference's SurfaceNearest
        (its backward is commented out, :17-49)"""
        self._need_mesh()
        if self._takes_device_route(points):
            ids, pts, _ = self._search_dev(points, _autograd.stream_of(points))
            return pts, ids
        pts, ids, _ = self._scan.nearest_points(_to_np(points, np.float32).reshape(-1, 3))
        return self._back(points, pts, ids)

    def nearest_points_with_coefficients(self, points):
        """the third output of the kernel (`coeff`, :10-14), which the reference's wrapper drops"""
        self._need_mesh()
        if self._takes_device_route(points):
            ids, pts, bary = self._search_dev(points, _autograd.stream_of(points), with_coefficients=True)
            return pts, ids, bary
        pts, ids, bary = self._scan.nearest_points(_to_np(points, np.float32).reshape(-1, 3))
        return self._back(points, pts, ids, bary)

    def inside_mesh(self, points):
        """:86-91 -> float32[n]: +1 inside, -1 outside"""
        self._need_mesh()
        return self._back(points, self._scan.inside_mesh(_to_np(points, np.float32).reshape(-1, 3)))[0]

    def intersects_any(self, origins, directions):
        """:93-99 -> bool[n]"""
        self._need_mesh()
        o = _to_np(origins, np.float32).reshape(-1, 3)
        return self._back(origins, self._scan.intersects_any(o, _to_np(directions, np.float32).reshape(-1, 3)))[0]
