"""Where body models and the GMM prior come from.

The reference reads `data/smpl/*.pkl` through smplx, `data/J_regressor_extra.npy` and
`data/gmm_08.pkl` relative to the working directory (config.py:1-6, smplify/prior.py:124-128), once
per *frame*.  Here a model is resolved once per process and cached per (type, gender, device):

  1. a dict registered with `register_model(...)` (tests, synthetic benchmarks),
  2. the files the reference itself opens - `data/smpl/SMPL_{GENDER}.pkl` + `data/J_regressor_extra.npy` (config.py:1-4,
     models/smpl.py:56-66) or `data/smplx/SMPLX_{GENDER}.npz` (smplify.py:63-80) - converted as smplx converts them
     (`model_files`),
  3. an `.npz` already in this package's tensor layout under `data/` (`{type}_{gender}.npz`),
  4. otherwise a clear error - nothing is downloaded and nothing is silently replaced.

age='kid' (SMPL only) is the adult model with the kid template's 11th shape direction (`model_files.kid_model`); the template is
the one registered with `register_kid_template(...)`, else the file at `kid_template_path` (default `data/smil/smil_web.pkl`,
config.SMIL_MODEL_DIR).  Kid models are cached under (type, gender, 'kid'); the adult keys are those of before.

The HMR weights of the initial estimate (`hmr.HMR`) are the state dict registered with `register_hmr(...)`, else the reference's
`data/model_checkpoint.pt` + `data/smpl_mean_params.npz` (config.HMR_CHECKPOINT, config.SMPL_MEAN_PARAMS), folded and packed once.

The OpenPose body weights (`openpose.OpenPose`) are the state dict registered with `register_openpose(...)`, else the reference's
`models/body_pose_model.pth` (openpose/infer_openpose.py:53), packed once; the hand weights (`openpose_hand.OpenPoseHand`) likewise
`register_openpose_hand(...)`, else `models/hand_pose_model.pth`.

The LBAM texture inpainter (`inpaint.Inpainter`, TextureFitting(inpaint=True)) takes the state dict registered with
`register_inpainter(...)`, else `external/LBAM_NoBN_ParisStreetView.pth` relative to the working directory (texture_fitting.py:189).
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from . import model_files

_MODELS = {}
_GMM = {}
_DEVICE_MODELS = {}
_KID_TEMPLATE = {}
_HMR = {}
HMR_CHECKPOINT = "model_checkpoint.pt"          # config.HMR_CHECKPOINT / SMPL_MEAN_PARAMS, in the data folder of the model files
SMPL_MEAN_PARAMS = "smpl_mean_params.npz"
_OPENPOSE = {}
OPENPOSE_WEIGHTS = os.path.join("models", "body_pose_model.pth")      # infer_openpose.py:53, relative to the working directory
_OPENPOSE_HAND = {}
OPENPOSE_HAND_WEIGHTS = os.path.join("models", "hand_pose_model.pth")  # next to the body weights
_INPAINTER = {}
INPAINTER_WEIGHTS = os.path.join("external", "LBAM_NoBN_ParisStreetView.pth")   # texture_fitting.py:189, relative to the working directory


class InpainterWeightsMissing(FileNotFoundError, NotImplementedError):
    """No LBAM weights: the reference's torch.load raises FileNotFoundError here; NotImplementedError as well, for callers that
    treated TextureFitting(inpaint=True) as unavailable"""


def _drop_kid(model_type=None, gender=None):
    """forget the kid models (and their device models) built from the given adult model (None: from any)"""
    for cache in (_MODELS, _DEVICE_MODELS):
        for k in [k for k in cache if k[-1] == "kid" and (model_type is None or k[:2] == (model_type, gender))]:
            v = cache.pop(k)
            if cache is _DEVICE_MODELS:
                v.close()


def register_model(model, model_type="smpl", gender="neutral"):
    _MODELS[(model_type, gender)] = model
    for k in [k for k in _DEVICE_MODELS if k[:2] == (model_type, gender)]:
        _DEVICE_MODELS.pop(k).close()
    _drop_kid(model_type, gender)


def register_kid_template(template):
    """the kid template [NV, 3] to use instead of the file (tests, synthetic benchmarks); None forgets it"""
    if template is None:
        _KID_TEMPLATE.clear()
    else:
        _KID_TEMPLATE["template"] = np.asarray(template, np.float32).copy()
    _drop_kid()


def get_kid_template(path=None):
    if "template" in _KID_TEMPLATE:
        return _KID_TEMPLATE["template"]
    return model_files.load_kid_template(model_files.KID_TEMPLATE_PATH if path is None else path)


def register_gmm(gmm):
    _GMM["gmm"] = gmm
    for k in list(_DEVICE_MODELS):
        _DEVICE_MODELS.pop(k).close()


def _load_npz_model(model_type, gender, folder="data"):
    for name in (f"{model_type}_{gender}.npz", f"{model_type}/{model_type.upper()}_{gender.upper()}.npz"):
        path = os.path.join(folder, name)
        if os.path.exists(path):
            z = np.load(path, allow_pickle=True)
            model = {k: z[k] for k in z.files}
            model.setdefault("model_type", model_type)
            extra = os.path.join(folder, "J_regressor_extra.npy")       # config.py:1
            if "J_regressor_extra" not in model and os.path.exists(extra):
                model["J_regressor_extra"] = np.load(extra)
            return model
    return None


def _check_age(model_type, age):
    if age not in ("adult", "kid"):
        raise ValueError(f"unknown age {age!r}: 'adult' or 'kid'")
    if age == "kid" and model_type != "smpl":
        raise ValueError("age='kid' is SMPL only: the reference builds SMPL-X without a kid template (smplx.create gets no age) "
                         "and then feeds 11 betas to a 10-direction model, so there is no SMPL-X kid behaviour to reproduce")


def get_model(model_type="smpl", gender="neutral", age="adult", kid_template_path=None):
    _check_age(model_type, age)
    if age == "kid":
        key = (model_type, gender, "kid")
        if key not in _MODELS:
            _MODELS[key] = model_files.kid_model(get_model(model_type, gender), get_kid_template(kid_template_path))
        return _MODELS[key]
    for key in ((model_type, gender), (model_type, "neutral")):
        if key in _MODELS:
            return _MODELS[key]
    model = model_files.load(model_type, gender)
    if model is None:
        model = _load_npz_model(model_type, gender)
    if model is None:
        official = "data/smpl/SMPL_%s.pkl + data/J_regressor_extra.npy" % gender.upper() if model_type == "smpl" else "data/smplx/SMPLX_%s.npz" % gender.upper()
        raise FileNotFoundError(
            f"no {model_type}/{gender} body model: place {official} (the files the reference reads) next to the working "
            f"directory, or register a model dict with bodyfitting_amd.assets.register_model()")
    _MODELS[(model_type, gender)] = model
    return model


def get_gmm(prior_folder="data", num_gaussians=8):
    if "gmm" in _GMM:
        return _GMM["gmm"]
    path = os.path.join(prior_folder, "gmm_{:02d}.pkl".format(num_gaussians))    # prior.py:122-124
    if not os.path.exists(path):
        raise FileNotFoundError(f"GMM prior {path!r} not found and none registered (assets.register_gmm)")
    with open(path, "rb") as f:
        gmm = pickle.load(f, encoding="latin1")
    _GMM["gmm"] = {k: np.asarray(gmm[k]) for k in ("means", "covars", "weights")}
    return _GMM["gmm"]


def gmm_buffers(gmm):
    """The three buffers the merged GMM NLL uses (reference smplify/prior.py:143-160).

    Returns float32 ``means[M,D]``, ``precisions[M,D,D]`` and ``nll_weights[M]`` computed in
    float64 and rounded once, exactly as the reference constructor does.
    """
    means = np.asarray(gmm["means"], dtype=np.float32)
    covs32 = np.asarray(gmm["covars"], dtype=np.float32)
    precisions = np.stack([np.linalg.inv(c) for c in covs32]).astype(np.float32)
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in gmm["covars"]])
    const = (2.0 * np.pi) ** (69 / 2.0)
    nll_weights = np.asarray(gmm["weights"] / (const * (sqrdets / sqrdets.min())))
    return means, precisions, nll_weights.astype(np.float32)


def shape_space_counts(model):
    """(num_betas, num_expression_coeffs) of an SMPL-X model dict: "num_betas" (absent: 10) shape columns, expression behind them"""
    nb = int(model.get("num_betas", 10))
    return nb, int(np.asarray(model["shapedirs"]).shape[2]) - nb


def shape_space_model(model_type, gender, num_betas, num_expression_coeffs):
    """The SMPL-X model dict with exactly these counts: the registered (or loaded) one when it has them; that dict's columns sliced
    when it holds at least as many of both; else the model file read again for them (model_files.load_smplx).  Nothing is clamped:
    a source without the columns is a ValueError that says what it holds."""
    base = get_model(model_type, gender)
    nb0, ne0 = shape_space_counts(base)
    nb, ne = int(num_betas), int(num_expression_coeffs)
    if (nb, ne) == (nb0, ne0):
        return base
    if nb < 10 or ne < 0:
        raise ValueError(f"num_betas={nb}, num_expression_coeffs={ne}: at least 10 betas and no negative count")
    if nb <= nb0 and ne <= ne0:
        sd = np.asarray(base["shapedirs"])
        out = dict(base, shapedirs=np.ascontiguousarray(np.concatenate([sd[:, :, :nb], sd[:, :, nb0:nb0 + ne]], axis=2)))
        out["num_betas"] = nb
        return out
    model = model_files.load(model_type, gender, num_betas=nb, num_expression_coeffs=ne)
    if model is None:
        raise ValueError(f"num_betas={nb}, num_expression_coeffs={ne}: the {model_type}/{gender} model at hand holds {nb0} shape and {ne0} "
                         f"expression directions and there is no model file to read more from")
    return model


def get_device_model(model_type="smpl", gender="neutral", device=0, age="adult", kid_template_path=None, num_betas=None,
                     num_expression_coeffs=None):
    """The HIP-resident model, created once per (type, gender, device) - (type, gender, device, 'kid') for a kid.
    num_betas / num_expression_coeffs (SMPL-X; None: the model's own): counts other than the model's own get a device model of their
    own under (type, gender, device, 'space', num_betas, num_expression_coeffs), built from `shape_space_model`."""
    from .native import DeviceModel
    _check_age(model_type, age)
    if num_betas is not None or num_expression_coeffs is not None:
        if model_type != "smplx":
            raise ValueError("num_betas / num_expression_coeffs: SMPL-X only (models.smpl.SMPL keeps the model's own betas)")
        nb0, ne0 = shape_space_counts(get_model(model_type, gender))
        nb, ne = nb0 if num_betas is None else int(num_betas), ne0 if num_expression_coeffs is None else int(num_expression_coeffs)
        if (nb, ne) != (nb0, ne0):
            key = (model_type, gender, int(device), "space", nb, ne)
            if key not in _DEVICE_MODELS:
                _DEVICE_MODELS[key] = DeviceModel(shape_space_model(model_type, gender, nb, ne), get_gmm(), device=device)
            return _DEVICE_MODELS[key]
    key = (model_type, gender, int(device)) + (("kid",) if age == "kid" else ())
    if key not in _DEVICE_MODELS:
        _DEVICE_MODELS[key] = DeviceModel(get_model(model_type, gender, age, kid_template_path), get_gmm(), device=device)
    return _DEVICE_MODELS[key]


def register_hmr(state_dict, mean_params=None):
    """HMR weights held in memory (tests, callers that load them themselves): a state dict as the checkpoint's 'model' entry and,
    when it lacks init_pose / init_shape / init_cam, the mean parameters (dict with pose[144], shape[10], cam[3]).  None forgets
    them.  Matched as the reference matches `model_checkpoint.pt` (unexpected keys ignored)."""
    _HMR.clear()
    if state_dict is not None:
        from . import hmr
        _HMR["packed"] = hmr.fold_and_pack(hmr.match_state(state_dict, HMR_CHECKPOINT, mean_params))


def hmr_paths(folder="data"):
    return os.path.join(folder, HMR_CHECKPOINT), os.path.join(folder, SMPL_MEAN_PARAMS)


def get_hmr(folder="data"):
    """-> (packed float32 weights, mean state float32[157]) for hmr.HMR, read once per process"""
    if "packed" in _HMR:
        return _HMR["packed"]
    from . import hmr
    ckpt, npz = hmr_paths(folder)
    if not (os.path.exists(ckpt) and os.path.exists(npz)):
        raise ValueError(f"no initial estimate: HMR needs {ckpt} and {npz} (the reference's config.HMR_CHECKPOINT and "
                         f"config.SMPL_MEAN_PARAMS), or weights registered with assets.register_hmr(); alternatively pass "
                         f"net_output=(betas[1,10], pose[1,72]) or set options.init_estimator")
    z = np.load(npz)
    mean = {k: z[k] for k in ("pose", "shape", "cam")}
    state = hmr.load_checkpoint(ckpt)["model"]
    _HMR["packed"] = hmr.fold_and_pack(hmr.match_state(state, ckpt, mean))
    return _HMR["packed"]


def register_openpose(state_dict):
    """OpenPose body weights held in memory (tests, callers that load them themselves): a state dict with the caffe keys of
    body_pose_model.pth (`conv1_1.weight`, ..., `Mconv7_stage6_L2.bias`).  None forgets them.  A missing key raises ValueError."""
    _OPENPOSE.clear()
    if state_dict is not None:
        from . import openpose
        _OPENPOSE["packed"] = openpose.pack(openpose.match_state(state_dict))


def get_openpose(path=None):
    """-> the packed float32 weights for openpose.OpenPose, read once per process"""
    if "packed" in _OPENPOSE:
        return _OPENPOSE["packed"]
    from . import openpose
    path = path or OPENPOSE_WEIGHTS
    if not os.path.exists(path):
        raise ValueError(f"no body keypoint estimator: OpenPose needs {path} (the reference's body_pose_model.pth) or weights "
                         f"registered with assets.register_openpose(); alternatively pass keypoints=")
    _OPENPOSE["packed"] = openpose.pack(openpose.load_weights(path))
    return _OPENPOSE["packed"]


def register_openpose_hand(state_dict):
    """OpenPose hand weights held in memory: a state dict with the caffe keys of hand_pose_model.pth (`conv1_1.weight`, ...,
    `Mconv7_stage6.bias`).  None forgets them.  A missing key raises ValueError."""
    _OPENPOSE_HAND.clear()
    if state_dict is not None:
        from . import openpose_hand
        _OPENPOSE_HAND["packed"] = openpose_hand.pack_hand(openpose_hand.match_hand_state(state_dict))


def get_openpose_hand(path=None):
    """-> the packed float32 weights for openpose_hand.OpenPoseHand, read once per process"""
    if "packed" in _OPENPOSE_HAND:
        return _OPENPOSE_HAND["packed"]
    from . import openpose_hand
    path = path or OPENPOSE_HAND_WEIGHTS
    if not os.path.exists(path):
        raise ValueError(f"no hand keypoint estimator: OpenPose hands need {path} (the reference's hand_pose_model.pth) or weights "
                         f"registered with assets.register_openpose_hand(); alternatively pass keypoints=")
    _OPENPOSE_HAND["packed"] = openpose_hand.pack_hand(openpose_hand.load_hand_weights(path))
    return _OPENPOSE_HAND["packed"]


def register_inpainter(state_dict):
    """LBAM inpainting weights held in memory: a state dict with LBAMModel(4, 3)'s keys (`ec1.conv.conv.weight`, ...,
    `dc7.weight`).  None forgets them.  A missing or unexpected key raises ValueError."""
    _INPAINTER.clear()
    if state_dict is not None:
        from . import inpaint
        _INPAINTER["packed"] = inpaint.pack(inpaint.match_state(state_dict))


def get_inpainter(path=INPAINTER_WEIGHTS):
    """-> the packed float32 weights for inpaint.Inpainter, read once per process: the registered ones, else `path`"""
    if "packed" in _INPAINTER:
        return _INPAINTER["packed"]
    from . import inpaint
    if not os.path.exists(path):
        raise InpainterWeightsMissing(f"no texture inpainter: TextureFitting(inpaint=True) needs {path} (the reference's LBAM "
                                      f"weights) or weights registered with assets.register_inpainter() (DESIGN.md section 14)")
    _INPAINTER["packed"] = inpaint.pack(inpaint.load_weights(path))
    return _INPAINTER["packed"]
