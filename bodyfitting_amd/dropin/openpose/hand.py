"""openpose/hand.py: `Hand(model_path)(oriImg) -> peaks [21, 2] int64` (x, y in oriImg's pixels), with the network, the maps, the
Gaussian filter and the component pick on the GPU (bodyfitting_amd.openpose_hand.OpenPoseHand)."""
import numpy as np

from bodyfitting_amd import openpose as _op
from bodyfitting_amd import openpose_hand as _oh


class Hand(object):
    def __init__(self, model_path, device=0):
        self.model_path = model_path
        self.device = device
        self._net = None

    def _estimator(self, shape):
        H, W = shape[:2]
        if self._net is None or H > self._net.max_h or W > self._net.max_w:
            if self._net is not None:
                self._net.close()
            self._net = _oh.OpenPoseHand(self.model_path, device=self.device, max_hands=1, max_h=max(H, 1024), max_w=max(W, 1024))
        return self._net

    def __call__(self, oriImg):
        """oriImg: uint8 BGR crop [h, w, 3] -> np.array([[x, y], ...]) int64 [21, 2]; [0, 0] where the thresholded map is empty"""
        img = np.ascontiguousarray(_op.check_image(oriImg))
        h, w = img.shape[:2]
        return self._estimator(img.shape).detect([img], [(0, 0, 0, w, h)])[0][0]
