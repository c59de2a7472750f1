"""age='kid' on the CPU: the kid model construction (smplx's SMPL kid branch), the template readers, the refusals, and the
gather of the 87-wide kid parameter vectors over gloo.  No GPU."""
import os
import pickle
import socket
import sys
import types

import numpy as np
import pytest
import torch

from bodyfitting_amd import assets, model_files, shard, synthetic as S
from oracle import smplify_oracle as O


@pytest.fixture(scope="module")
def adult():
    return S.make_model("smpl", seed=0)


@pytest.fixture(scope="module")
def template(adult):
    return S.make_kid_template(adult)


def _smplx_kid_branch(v_template, shapedirs, kid_template):
    """the published smplx SMPL.__init__ kid branch, restated: centre the kid template, append (it - v_template) as direction 11"""
    v_template_smil = np.asarray(kid_template, np.float64)
    v_template_smil -= np.mean(v_template_smil, axis=0)
    v_template_diff = np.expand_dims(v_template_smil.astype(np.float32) - v_template, axis=2)
    return np.concatenate((shapedirs[:, :, :10], v_template_diff), axis=2)


def test_kid_model_is_the_smplx_kid_branch(adult, template):
    kid = model_files.kid_model(adult, template)
    want = _smplx_kid_branch(adult["v_template"], adult["shapedirs"], template)
    assert kid["shapedirs"].shape == (6890, 3, 11) and kid["shapedirs"].dtype == np.float32
    np.testing.assert_array_equal(kid["shapedirs"], want)
    for k in adult:                                  # nothing else of the model changes
        if k != "shapedirs":
            assert kid[k] is adult[k], k
    assert adult["shapedirs"].shape == (6890, 3, 10)


def test_eleventh_beta_gives_the_centred_kid_template(adult, template):
    """known answer: betas = e_10 at zero pose -> v_template + (t - v_template) = the centred kid template"""
    kid = model_files.kid_model(adult, template)
    m = O.to_torch_model(kid, torch.float64)
    betas = torch.zeros(1, 11, dtype=torch.float64)
    betas[0, 10] = 1.0
    out = O.smpl_forward(m, betas, torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 69, dtype=torch.float64))
    t = np.asarray(template, np.float64)
    centred = (t - t.mean(0)).astype(np.float32)
    np.testing.assert_allclose(out["vertices"][0].numpy(), centred, atol=1e-6)
    # ... and the joints follow through J_regressor on the shaped mesh
    np.testing.assert_allclose(out["joints_ori"][0, :24].numpy(), np.asarray(kid["J_regressor"], np.float64) @ centred, atol=1e-6)
    # zero betas: the adult template, as before
    out0 = O.smpl_forward(m, torch.zeros(1, 11, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 69, dtype=torch.float64))
    np.testing.assert_allclose(out0["vertices"][0].numpy(), adult["v_template"], atol=1e-6)


def test_kid_template_npy_and_pickle_readers(tmp_path, template):
    p = tmp_path / "kid.npy"
    np.save(p, template)
    np.testing.assert_array_equal(model_files.load_kid_template(str(p)), template)
    # the SMIL pickle: v_template as a chumpy array, read without chumpy
    mod, sub = types.ModuleType("chumpy"), types.ModuleType("chumpy.ch")

    class Ch:
        def __init__(self, x):
            self.x = x
    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    sub.Ch = Ch
    mod.ch = sub
    sys.modules["chumpy"], sys.modules["chumpy.ch"] = mod, sub
    try:
        payload = pickle.dumps({"v_template": Ch(template.astype(np.float64)), "f": np.zeros((2, 3), np.int64)}, protocol=2)
    finally:
        del sys.modules["chumpy"], sys.modules["chumpy.ch"]
    q = tmp_path / "smil_web.pkl"
    q.write_bytes(payload)
    got = model_files.load_kid_template(str(q))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, template)
    # a plain (cleaned) pickle too
    r = tmp_path / "plain.pkl"
    r.write_bytes(pickle.dumps({"v_template": template}))
    np.testing.assert_array_equal(model_files.load_kid_template(str(r)), template)
    with pytest.raises(FileNotFoundError):
        model_files.load_kid_template(str(tmp_path / "absent.pkl"))
    bad = tmp_path / "bad.pkl"
    bad.write_bytes(pickle.dumps({"weights": template}))
    with pytest.raises(ValueError):
        model_files.load_kid_template(str(bad))


def test_kid_template_of_another_topology_is_refused(adult, template, tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="does not match"):
        model_files.kid_model(adult, template[:-1])
    p = tmp_path / "short.npy"
    np.save(p, template[:100])
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "neutral"): adult})
    monkeypatch.setattr(assets, "_KID_TEMPLATE", {})
    with pytest.raises(ValueError, match="does not match"):
        assets.get_model("smpl", "neutral", "kid", kid_template_path=str(p))


def test_kid_model_through_assets(adult, template, tmp_path, monkeypatch):
    """the file at kid_template_path, or the registered template; cached under (type, gender, 'kid'); the adult key unchanged"""
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "neutral"): adult})
    monkeypatch.setattr(assets, "_KID_TEMPLATE", {})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    p = tmp_path / "kid.npy"
    np.save(p, template)
    kid = assets.get_model("smpl", "neutral", "kid", kid_template_path=str(p))
    assert kid["shapedirs"].shape[2] == 11
    assert assets.get_model("smpl", "neutral") is adult
    assert assets.get_model("smpl", "neutral", "kid") is kid
    assert set(assets._MODELS) == {("smpl", "neutral"), ("smpl", "neutral", "kid")}
    other = template * 0.9
    assets.register_kid_template(other)                 # a registered template replaces the file and drops the cached kid
    kid2 = assets.get_model("smpl", "neutral", "kid", kid_template_path=str(p))
    np.testing.assert_array_equal(kid2["shapedirs"], model_files.kid_model(adult, other)["shapedirs"])
    assets.register_kid_template(None)
    monkeypatch.chdir(tmp_path)                         # default path: data/smil/smil_web.pkl under the working directory
    with pytest.raises(FileNotFoundError, match="smil_web.pkl"):
        assets.get_model("smpl", "neutral", "kid")
    os.makedirs("data/smil")
    with open("data/smil/smil_web.pkl", "wb") as f:
        pickle.dump({"v_template": template}, f)
    np.testing.assert_array_equal(assets.get_model("smpl", "neutral", "kid")["shapedirs"], kid["shapedirs"])


def test_smplx_kid_is_refused_before_any_device_work(monkeypatch):
    from bodyfitting_amd.smplify import SMPLify
    called = []
    monkeypatch.setattr(assets, "get_device_model", lambda *a, **k: called.append(a))
    with pytest.raises(ValueError, match="SMPL-X|smplx"):
        SMPLify(smpl_type="smplx", age="kid")
    with pytest.raises(ValueError):
        SMPLify(smpl_type="smpl", age="teen")
    assert not called
    with pytest.raises(ValueError, match="SMPL only"):
        assets.get_model("smplx", "neutral", "kid")
    with pytest.raises(ValueError):
        model_files.kid_model({"model_type": "smplx", "v_template": np.zeros((3, 3)), "shapedirs": np.zeros((3, 3, 20))}, np.zeros((3, 3)))


def test_kid_problem_model_folds_the_eleventh_beta(adult, template):
    """the synthetic kid problems' GT: 10 drawn betas on the folded model == the same betas plus the kid beta on the kid model"""
    kid = model_files.kid_model(adult, template)
    folded = S.kid_problem_model(kid, 0.4)
    b = np.random.default_rng(0).normal(0.0, 0.5, 10)
    pose = np.random.default_rng(1).normal(0.0, 0.2, 72)
    v1, j1 = S.smpl_joints64(folded, b, pose)
    v2, j2 = S.smpl_joints64(kid, np.concatenate([b, [0.4]]), pose)
    np.testing.assert_allclose(v1, v2, atol=1e-6)
    np.testing.assert_allclose(j1, j2, atol=1e-6)


def _params87(frames):
    return (np.stack([np.arange(87, dtype=np.float32) + 1000.0 * f for f in frames]) if len(frames)
            else np.zeros((0, 87), np.float32))


def _worker87(rank, world, port, n_frames, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard.shard_range(n_frames, rank, world)
    send = torch.from_numpy(shard.pad_block(_params87(range(lo, hi)), n_frames, world))
    recv = torch.empty(world * send.numel())
    dist.all_gather_into_tensor(recv, send.reshape(-1))
    np.save(os.path.join(out, f"r{rank}.npy"), shard.unpack(recv.numpy().reshape(world, *send.shape), n_frames, world))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_frames", [7, 8])
def test_gather_of_kid_parameters_world2_gloo(tmp_path, n_frames):
    """a kid parameter vector is 87 wide (3 + 1 + 69 + 11 + 3): the gather's pad / unpack bookkeeping in libbodyfit takes it"""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker87, args=(2, port, n_frames, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        np.testing.assert_array_equal(np.load(tmp_path / f"r{r}.npy"), _params87(range(n_frames)))


def test_split_params_of_a_kid_vector():
    from bodyfitting_amd.native import pack_params, split_params
    p = np.arange(87, dtype=np.float32)
    d = split_params(p, 24, 11)
    assert d["betas"].shape == (11,) and d["global_orient"].tolist() == [84.0, 85.0, 86.0]
    np.testing.assert_array_equal(pack_params(d), p)
