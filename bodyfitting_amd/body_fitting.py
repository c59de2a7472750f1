"""`smplify.body_fitting.BodyFitting` of the reference (smplify/body_fitting.py:44-107) on the HIP path.

Keeps `__init__(options)` / `__call__(images, c2ws, Ks, keypoints, gender=..., keyframe=..., use_frames=...,
use_mask=..., masks=..., mask_frames=..., render_skip=..., output_folder=..., use_mesh=..., meshfile=...,
disp=...)` and the files it writes (`{smpl_type}_parameter.npy` = pickled result dict, `{smpl_type}.obj`).
The initial (betas, pose) come from the `net_output=` keyword, else from `options.init_estimator(image, c2w)`, else - as in
the reference (body_fitting.py:57-75,86) - from HMR on `images[keyframe]` / `c2ws[keyframe]` (`hmr.HMR`, on the GPU; weights from
`assets.get_hmr()`, one network per BodyFitting).
Without `keypoints` (None) the 2-D keypoints come from the reference's OpenPose body estimator on the GPU (`openpose.OpenPose`,
weights from `assets.get_openpose()`), in place of apps/genebody_fitting.py's openpose.bin run: each view's image (RGB, as the
runner loads it) is flipped to BGR - what openpose.bin reads from the written PNG - detected, laid out as BODY_25 as
openpose/infer_openpose.py lays it out, and the person io.load_openpose would pick is kept.
With `options.detect_hands` (default False) and smpl_type 'smplx', the hands come too, as `openpose.bin --hand` gives them
(apps/genebody_fitting.py:144-155): the reference's hand estimator (`openpose_hand.OpenPoseHand`, weights from
`assets.get_openpose_hand()`) on every box util.handDetect accepts, all views of the frame in one batched call; each person gets
`hand_left` / `hand_right` [21, 3] in image coordinates, and the person is picked by the confidence sum over all its arrays.
"""
from __future__ import annotations

import os

import numpy as np

from .io import save_obj_mesh
from .smplify import SMPLify


class BodyFitting:
    def __init__(self, options):
        self.options = options
        self.debug = getattr(options, "debug", False)
        self.loadsize = getattr(options, "load_size", 512)
        self.use_mask = getattr(options, "use_mask", False)
        self.smpl_type = getattr(options, "smpl_type", "smpl")
        self.use_hand_face = self.smpl_type == "smplx"
        self.init_estimator = getattr(options, "init_estimator", None)
        self.num_iters = getattr(options, "num_iters", 600)            # smplify.py:26 default
        self._fitters = {}
        self._hmr = None
        self._openpose = None
        self._openpose_hand = None
        self.detect_hands = bool(getattr(options, "detect_hands", False)) and self.smpl_type == "smplx"

    def _fitter(self, gender):
        if gender not in self._fitters:      # the reference rebuilds this per call (body_fitting.py:82)
            self._fitters[gender] = SMPLify(smpl_type=self.smpl_type, age=getattr(self.options, "age", "adult"),
                                            gender=gender, use_mask=self.use_mask, num_iters=self.num_iters,
                                            device=getattr(self.options, "device", 0), debug=False)
        return self._fitters[gender]

    def run_hmr(self, image, c2w):
        """body_fitting.py:57-75: (pred_betas [1, 10], pred_poses [1, 72]) of one image, root rotation taken to world by c2w"""
        if self._hmr is None:                 # (no weights registered and no files: ValueError naming the two files)
            from .hmr import HMR
            self._hmr = HMR(device=getattr(self.options, "device", 0), max_batch=1)
        return self._hmr.predict([image], None if c2w is None else np.asarray(c2w)[None])

    def detect_keypoints(self, images):
        """per view {'pose': [25, 3]} of the person io.load_openpose would choose from infer_openpose.py's JSON, or None"""
        from . import openpose as O
        if images is None:
            raise ValueError("BodyFitting: keypoints=None detects them on the images, and images is None")
        bgr = [np.ascontiguousarray(np.asarray(im)[:, :, ::-1]) for im in images]
        H, W = bgr[0].shape[:2]
        if self._openpose is None:            # (no weights registered and no file: ValueError naming models/body_pose_model.pth)
            self._openpose = O.OpenPose(device=getattr(self.options, "device", 0), max_batch=4, max_h=max(H, 1024), max_w=max(W, 1024))
        if not self.detect_hands:
            return [O.select_person(p) for p in self._openpose.pose25(bgr)]
        from . import openpose_hand as OH
        if self._openpose_hand is None:       # (no weights registered and no file: ValueError naming models/hand_pose_model.pth)
            self._openpose_hand = OH.OpenPoseHand(device=getattr(self.options, "device", 0), max_hands=16, max_h=max(H, 1024),
                                                  max_w=max(W, 1024))
        return [OH.select_person_entry(p) for p in OH.detect_people(self._openpose, self._openpose_hand, bgr)]

    def __call__(self, images, c2ws, Ks, keypoints=None, gender="male", keyframe=25, use_frames=list(range(48)),
                 use_mask=False, masks=None, mask_frames=None, render_skip=12, output_folder=None,
                 use_mesh=False, meshfile=None, disp=False, net_output=None):
        if net_output is None:
            if self.init_estimator is not None:
                net_output = self.init_estimator(images[keyframe], c2ws[keyframe])
            else:
                net_output = self.run_hmr(images[keyframe], c2ws[keyframe])
        if keypoints is None:
            keypoints = self.detect_keypoints(images)
        imsize = images[0].shape[0] if images is not None else self.loadsize
        result = self._fitter(gender)(net_output, c2ws, Ks, keypoints, output_folder, use_mask=use_mask, masks=masks,
                                      use_frames=use_frames, mask_frames=mask_frames, keyframe=keyframe, imsize=imsize,
                                      use_mesh=use_mesh, meshfile=meshfile, displacement=disp)
        if output_folder is not None:
            os.makedirs(output_folder, exist_ok=True)
            np.save(os.path.join(output_folder, f"{self.smpl_type}_parameter.npy"), result)
            save_obj_mesh(os.path.join(output_folder, f"{self.smpl_type}.obj"), result["vertices"], result["faces"])
            if disp and "displacement" in result:                                    # body_fitting.py:98-99
                save_obj_mesh(os.path.join(output_folder, f"{self.smpl_type}+d.obj"),
                              result["vertices"] + result["displacement"], result["faces"])
        return result
