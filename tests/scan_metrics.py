"""End-state metrics of the scan loops against the scan, shared by the config-5 tests (tests/test_gpu_scan.py at the reduced model,
tests/test_gpu_configs_full.py at the stated size).  Computed on the CPU by the oracle's pieces; nothing here touches the GPU."""
import numpy as np

from oracle import mesh_oracle as MO


def disp_metrics(model, sv, sf, base, disp):
    """end-state metrics of the SMPL+D stage (smplify.py:228-247) for `base + disp` against the scan, by the oracle's
    pieces: distribution of point-to-scan distances, the icp term, normal and laplacian energies"""
    import torch
    P = (base + disp).astype(np.float32)
    ids, cp, _ = MO.ReferenceSearcher(sv, sf).nearest(P)
    d = np.linalg.norm(P - cp, axis=1)
    faces_t = torch.as_tensor(np.asarray(model["faces"]), dtype=torch.long)
    norms = MO.compute_normal_torch(torch.tensor(P, dtype=torch.float64), faces_t)
    tris = sv.astype(np.float64)[sf]
    fn = torch.tensor(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(np.float32), dtype=torch.float64)
    return {"mean": float(d.mean()), "median": float(np.median(d)), "p95": float(np.percentile(d, 95)), "icp": float(np.linalg.norm(P - cp)),
            "normal": float(MO.normal_loss(fn[torch.as_tensor(ids, dtype=torch.long)], norms)),
            "laplacian": float(MO.normal_laplacian_smoothness(norms, faces_t))}
