"""The device route at a wide SMPL-X shape space in a FRESH process (tests/test_gpu_smplx_shape_space.py).  Like
tests/device_route_child.py this module imports torch FIRST and the library only inside its function, so that both share one HIP
runtime.  The yardstick is the host route on the same build, which tests/test_gpu_smplx_shape_space.py holds to the float64 oracle:
the device route issues the same launches - the pack and join kernels included - and must give the same bits."""
import numpy as np
import torch                    # (first: see above)

from device_route_child import GPU, XINPUTS, _cot, _equal, _gpu, _repo, _smplx_params, _took, _two_calls, _guarded, _guarded_is
from lanes_child import _run

NB, NE = 16, 50


def _params(n, seed):
    p = _smplx_params(n, seed)
    rng = np.random.default_rng(seed + 77000)
    p["betas"] = np.ascontiguousarray(np.concatenate([p["betas"], rng.normal(0, 0.7, (n, NB - 10)).astype(np.float32)], axis=1))
    p["expression"] = np.ascontiguousarray(np.concatenate([p["expression"], rng.normal(0, 0.7, (n, NE - 10)).astype(np.float32)], axis=1))
    return p


def same_bits(out_path):
    def body():
        _repo()
        from bodyfitting_amd import assets, native as N, synthetic as S
        from bodyfitting_amd import smplx as X
        _took("device")
        model = S.widen_shape_space(S.make_model("smplx", seed=0, nv=1200), NB, NE, seed=0)
        assets._MODELS.clear(); assets._DEVICE_MODELS.clear()
        assets._MODELS[("smplx", "neutral")] = model
        assets._GMM["gmm"] = S.make_gmm(seed=0)
        drop = X.create(model_type="smplx", use_face_contour=True, num_betas=NB, num_expression_coeffs=NE)
        dev = drop._dev
        assert (dev.n_betas, dev.n_expression, dev.shape_ext_wide) == (NB, NE, True)
        names = XINPUTS + ("expression",)
        arg = {"vertices": "dverts", "joints": "djoints_all", "full_pose": "dfull_pose"}
        before = N.dev_route_stats()
        for n in (1, 9, 65):
            p = _params(n, 70 + n)
            ref = drop(**p, return_full_pose=True)
            shapes = {"vertices": (n, dev.n_verts, 3), "joints": (n, dev.n_joints_all, 3), "full_pose": (n, 3 * dev.n_joints)}
            cot = {k: _cot(s, 70 + n + i) for i, (k, s) in enumerate(shapes.items())}
            for keys in (("vertices",), ("joints",), tuple(shapes)):
                x = {k: _gpu(p[k]) for k in names}
                out = drop(**x, return_full_pose=True)
                for k in shapes:
                    assert getattr(out, k).device.type == "cuda"
                    _equal(getattr(out, k), getattr(ref, k), f"n={n} {k}")
                sum((getattr(out, k) * _gpu(cot[k], False)).sum() for k in keys).backward()
                want = dev.vjp_smplx(*[p[k] for k in XINPUTS], **{arg[k]: cot[k] for k in keys}, expression=p["expression"])
                assert want[0].shape == (n, NB) and want[8].shape == (n, NE)
                for k, w in zip(names, want):
                    _equal(x[k].grad, w, f"n={n} {keys} d{k}")
            # betas alone on the device: expression is a NULL pointer = zero coefficients
            few = {k: _gpu(p[k]) for k in ("betas", "global_orient", "body_pose")}
            _equal(drop(**few).vertices, drop(**{k: p[k] for k in few}).vertices, f"n={n} three blocks only")
        after = N.dev_route_stats()
        assert after["dev_calls"] > before["dev_calls"] and after["stream_switches"] == before["stream_switches"]
        # a repeated call of one shape allocates nothing: the pack's two blocks and the joined rows come from the workspace's slots
        n = 9
        p = _params(n, 79)
        x = {k: torch.tensor(p[k], device=GPU) for k in names}
        cotv = torch.tensor(_cot((n, dev.n_verts, 3), 5), device=GPU)
        want = dev.vjp_smplx(*[p[k] for k in XINPUTS], dverts=_cot((n, dev.n_verts, 3), 5), expression=p["expression"])
        stream = torch.cuda.current_stream().cuda_stream

        def forward():
            v, a = _guarded(n * dev.n_verts * 3)
            dev.forward_smplx_dev(n, stream, [x[k].data_ptr() for k in XINPUTS], expression=x["expression"].data_ptr(), vertices=a)
            torch.cuda.synchronize()
            return v

        def reverse():
            db, adb = _guarded(n * NB)
            de, ade = _guarded(n * NE)
            dev.vjp_smplx_dev(n, stream, [x[k].data_ptr() for k in XINPUTS], expression=x["expression"].data_ptr(), dverts=cotv.data_ptr(),
                              grads=[adb] + [0] * 7, dexpression=ade)
            torch.cuda.synchronize()
            return db, de

        v = _two_calls(forward, "forward_smplx_dev (16, 50)")
        _guarded_is(v, dev.forward_smplx(*[p[k] for k in XINPUTS], expression=p["expression"])["vertices"], "vertices")
        db, de = _two_calls(reverse, "vjp_smplx_dev (16, 50)")
        _guarded_is(db, want[0], "dbetas")
        _guarded_is(de, want[8], "dexpression")
        dev.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)
