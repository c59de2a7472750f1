"""The model variants the skinning-width and fit-lane tests share (tests/test_skinning_width.py, test_gpu_skinning_width.py,
test_gpu_lane_models.py and its child): how a model is sorted into the kernels' skinning paths, the table of variants with the class
and the fit instance each must land on, and their synthetic problems.  A plain module: no test, no fixture, no GPU call on import."""
import numpy as np

from bodyfitting_amd import model_files, synthetic as S

N_LOSS_JOINTS = {"smpl": 25, "smplx": 135}      # the keypoint loss's joints (native.model_desc)
KID_BETA = 0.4            # the ground truth's 11th beta of a kid variant's problems


def width_class(model):
    """(v_nnz, sel_nnz) as derive_tables sets them: the most bones of any vertex -> 4 / 8 / 0; the most of the selector vertices
    the routed keypoint loss reads (none when the loss is dense, more than 32 joints) -> that count if <= BF_SEL_NNZ = 8, else 0"""
    lw = np.asarray(model["lbs_weights"])
    nnz = (lw != 0).sum(1)
    most = int(nnz.max())
    nl = N_LOSS_JOINTS[model.get("model_type", "smpl")]
    jm = np.asarray(model["joint_map"])[:nl] if nl <= 32 else np.zeros(0, np.int64)
    sel = np.asarray(model["selector_ids"])[jm[jm >= lw.shape[1]] - lw.shape[1]]
    s = int(nnz[sel].max()) if len(sel) else 0
    return (4 if most <= 4 else 8 if most <= 8 else 0), (s if s <= 8 else 0)


def loss_selectors(model):
    """the selector vertices the SMPL keypoint loss reads (FitTab's selector rows), in joint-map order"""
    nj = np.asarray(model["lbs_weights"]).shape[1]
    jm = np.asarray(model["joint_map"])[:N_LOSS_JOINTS["smpl"]]
    return [int(v) for v in np.asarray(model["selector_ids"])[jm[jm >= nj] - nj]]


def quiet_vertex(model):
    """a vertex no selector and no regressor row touches: widening it moves v_nnz and nothing the fit's selector rows read"""
    busy = set(np.asarray(model["selector_ids"]).tolist())
    for k in ("J_regressor_extra", "J_regressor"):
        if k in model:
            busy |= set(np.nonzero(np.asarray(model[k]).any(0))[0].tolist())
    return next(v for v in range(np.asarray(model["v_template"]).shape[0]) if v not in busy)


# name -> (model type, nv, bones, override key, kid, expected (v_nnz, sel_nnz or a range), fit instance)
VARIANTS = {
    "smpl_B8": ("smpl", None, (5, 8), None, False, (8, (5, 8)), "table-driven"),
    "smpl_BD": ("smpl", None, (9, 12), None, False, (0, 0), "table-driven"),
    "smpl_4+1": ("smpl", None, 4, "quiet", False, (0, 4), "sized"),
    "smpl_4+S": ("smpl", None, 4, "selector", False, (8, 6), "table-driven"),
    "kid": ("smpl", None, 4, None, True, (4, 4), "table-driven"),          # the kid model of the default SMPL
    "kid_B8": ("smpl", None, (5, 8), None, True, (8, (5, 8)), "table-driven"),
    "smplx_4": ("smplx", None, 4, None, False, (4, 0), "table-driven"),
    "smplx_B8": ("smplx", None, (5, 8), None, False, (8, 0), "table-driven"),
    "smplx_BD": ("smplx", None, (9, 12), None, False, (0, 0), "table-driven"),
    "nv690_B8": ("smpl", 690, (5, 8), None, False, (8, (5, 8)), "table-driven"),
    "nv690_BD": ("smpl", 690, (9, 12), None, False, (0, 0), "table-driven"),
}


def build_model(name):
    kind, nv, bones, over, kid, _, _ = VARIANTS[name]
    wide = None
    if over:
        base = S.make_model(kind, nv=nv)
        wide = {quiet_vertex(base): 9} if over == "quiet" else {loss_selectors(base)[0]: 6}
    model = S.make_model(kind, seed=0, nv=nv, bones=bones, wide=wide)
    if kid:
        model = model_files.kid_model(model, S.make_kid_template(model))
    return model


class Variants:
    """the variants' models and device models, built on first use and checked for their class"""

    def __init__(self, gmm):
        self.gmm, self.models, self.devs, self.cache = gmm, {}, {}, {}

    def get(self, name):
        if name not in self.devs:
            from bodyfitting_amd import native as N
            model = build_model(name)
            want_class, want_instance = VARIANTS[name][5:]
            v_nnz, sel_nnz = width_class(model)
            assert v_nnz == want_class[0], (name, v_nnz)
            if isinstance(want_class[1], tuple):
                assert want_class[1][0] <= sel_nnz <= want_class[1][1], (name, sel_nnz)
            else:
                assert sel_nnz == want_class[1], (name, sel_nnz)
            dev = N.DeviceModel(model, self.gmm, device=0)
            assert dev.fit_instance == want_instance, (name, dev.fit_instance)
            self.models[name], self.devs[name] = model, dev
        return self.models[name], self.devs[name]

    def close(self):
        for d in self.devs.values():
            d.close()


def smpl_problem(name, model, frame=0, n_views=48, **kw):
    """synthetic.make_problem for an SMPL variant; a kid variant's has 11 initial betas and KID_BETA as the truth's 11th"""
    if VARIANTS[name][4]:
        return S.as_kid_problem(S.make_problem(S.kid_problem_model(model, KID_BETA), frame=frame, n_views=n_views, **kw), KID_BETA)
    return S.make_problem(model, frame=frame, n_views=n_views, **kw)
