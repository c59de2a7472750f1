"""openpose/body.py: `Body(model_path)(oriImg) -> (candidate, subset)` and `get_pose(candidate, subset)`, with the network, the maps,
the peaks and the limb scores on the GPU (bodyfitting_amd.openpose.OpenPose)."""
import numpy as np

from bodyfitting_amd import openpose as _op


def get_pose(candidate, subset):
    """body.get_pose: per person [18, 3] (x, y, score), zeros for missing parts"""
    return _op.get_pose(candidate, subset)


class Body(object):
    def __init__(self, model_path, device=0):
        self.model_path = model_path
        self.device = device
        self._net = None

    def _estimator(self, shape):
        H, W = shape[:2]
        if self._net is None or H > self._net.max_h or W > self._net.max_w:
            if self._net is not None:
                self._net.close()
            self._net = _op.OpenPose(self.model_path, device=self.device, max_batch=1, max_h=max(H, 1024), max_w=max(W, 1024))
        return self._net

    def __call__(self, oriImg):
        """oriImg: uint8 BGR [H, W, 3] -> (candidate [N, 4] = x, y, score, id; subset [P, 20])"""
        img = np.ascontiguousarray(oriImg)
        return self._estimator(img.shape).detect(img)
