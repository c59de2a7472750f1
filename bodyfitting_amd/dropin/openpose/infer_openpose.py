"""openpose/infer_openpose.py: `get_pose(oriImg, body_estimation)` returns the per-person COCO-17 poses [17, 3] as the reference
does; its drawing and cv2.imwrite are not reproduced (said once on stderr).  `openpose_json(poses)` / `write_json(path, poses)` give
the BODY_25-layout file the reference's __main__ writes."""
import numpy as np

from bodyfitting_amd import openpose as _op


def get_pose(oriImg, body_estimation):
    candidate, subset = body_estimation(oriImg)
    poses = [p[list(_op.COCO17_FROM_18)] for p in _op.get_pose(candidate, subset)]
    _op.warn_drawing("infer_openpose.get_pose's draw_bodypose / cv2.imwrite('results/OpenPose_inf.png')")
    return poses


def to_body25(poses):
    """infer_openpose.py:57-70: COCO-17 poses -> per person BODY_25 [25, 3] (float32 values)"""
    kpts = np.float32(np.array(poses).reshape([-1, 17, 3]))
    out = []
    for i in range(kpts.shape[0]):
        b25 = np.zeros((25, 3))
        b25[list(_op.BODY25_FROM_17)] = kpts[i]
        out.append(b25)
    return out


def write_json(path, poses):
    """the {"version": 1.3, "people": [...]} file of infer_openpose.py:71-82 for COCO-17 poses"""
    _op.write_json(path, to_body25(poses))
