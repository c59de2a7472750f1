"""bf_model_create on descriptors with one defect each: every defect is refused with its own status code and message, before
anything is uploaded (csrc/model_api.hip: check_desc)."""
import ctypes as C

import numpy as np
import pytest

from bodyfitting_amd import _lib
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S

INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def smplx_model():
    return S.make_model("smplx", seed=0)


def _with(model, key, edit):
    """a copy of `model` whose array `key` is a fresh copy changed by edit(array)"""
    out = dict(model)
    a = np.array(model[key], copy=True)
    edit(a)
    out[key] = a
    return out


def _create(model, gmm, edit_desc=None):
    """-> (status, bf_last_error text) of bf_model_create on device 0; a model that does get created is destroyed again"""
    lib = _lib.load()
    d, _, keep = N.model_desc(model, gmm)
    if edit_desc:
        edit_desc(d)
    h = C.c_void_p()
    rc = lib.bf_model_create(C.byref(d), 0, C.byref(h))
    msg = lib.bf_last_error().decode()
    if rc == 0:
        lib.bf_model_destroy(h)
    del keep
    return rc, msg


def _set(i, v):
    def edit(a):
        a.reshape(-1)[i] = v
    return edit


SMPL_CASES = {
    "root_parent": (lambda m: _with(m, "parents", _set(0, 0)), None, INVALID, "parents[0] must be -1"),
    "parent_order": (lambda m: _with(m, "parents", _set(5, 7)), None, INVALID, "parents[i] must be in [0,i)"),
    "seven_children": (lambda m: _with(m, "parents", lambda a: a.__setitem__(slice(1, 8), 0)), None, UNSUPPORTED,
                       "a joint has more than 6 children"),
    "selector_id": (lambda m: _with(m, "selector_ids", _set(3, 6890)), None, INVALID, "selector id out of range"),
    "joint_map_entry": (lambda m: _with(m, "joint_map", _set(30, 24 + 21 + 9)), None, INVALID, "joint_map entry out of range"),
    "loss_joint_on_extra": (lambda m: _with(m, "joint_map", _set(2, 24 + 21)), None, UNSUPPORTED,
                            "a loss joint maps to an extra-regressor joint"),
    "face_index": (lambda m: _with(m, "faces", _set(100, 6890)), None, INVALID, "face index out of range"),
    "negative_face_index": (lambda m: _with(m, "faces", _set(7, -1)), None, INVALID, "face index out of range"),
    "too_many_betas": (lambda m: m, lambda d: setattr(d, "n_betas", 13), UNSUPPORTED, "need 2..64 joints and 1..12 betas"),
    "gmm_shape": (lambda m: m, lambda d: setattr(d, "gmm_dim", 63), UNSUPPORTED, "the GMM prior must be 8 components x 69 dims"),
    "loss_joints": (lambda m: m, lambda d: setattr(d, "n_loss_joints", 50), UNSUPPORTED, "1..192 loss joints supported"),
}

SMPLX_CASES = {
    "landmark_face": (lambda m: _with(m, "lmk_faces_idx", _set(4, 20946)), None, INVALID, "landmark face out of range"),
    "dynamic_landmark_face": (lambda m: _with(m, "dynamic_lmk_faces_idx", _set(40, -2)), None, INVALID,
                              "dynamic landmark face out of range"),
    "face_index": (lambda m: _with(m, "faces", _set(9, 10475)), None, INVALID, "face index out of range"),
    "no_hand_pca": (lambda m: m, lambda d: setattr(d, "n_hand_pca", 0), INVALID, "incomplete SMPL-X description"),
    "no_pose_mean": (lambda m: m, lambda d: setattr(d, "pose_mean", None), INVALID, "incomplete SMPL-X description"),
    "dyn_rows": (lambda m: m, lambda d: setattr(d, "n_dyn_rows", 78), INVALID, "incomplete SMPL-X description"),
    "neck_joint": (lambda m: m, lambda d: setattr(d, "neck_joint", 55), INVALID, "incomplete SMPL-X description"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SMPL_CASES))
def test_smpl_descriptor_defect(case, smpl_model, gmm):
    make, edit_desc, code, text = SMPL_CASES[case]
    assert _create(make(smpl_model), gmm, edit_desc) == (code, "bf_model_create: " + text)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SMPLX_CASES))
def test_smplx_descriptor_defect(case, smplx_model, gmm):
    make, edit_desc, code, text = SMPLX_CASES[case]
    assert _create(make(smplx_model), gmm, edit_desc) == (code, "bf_model_create: " + text)


@pytest.mark.gpu
def test_sound_descriptors_create(smpl_model, smplx_model, gmm):
    assert _create(smpl_model, gmm)[0] == 0
    assert _create(smplx_model, gmm)[0] == 0
