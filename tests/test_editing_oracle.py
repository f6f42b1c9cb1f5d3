"""CPU tests of scene editing (per-point Rw2c frames): the torch restatement of the reference's per-point branch (tests/editing_case.py)
against the fixture generated from the reference's own PointAggregator (tests/golden/make_editing_golden.py), ``compose_parts`` against
a numpy restatement of run/editing.py:189-212, and the frame table through prune / grow_points / checkpoints."""
import numpy as np
import pytest
import torch

import editing_case as E
from cases import build_case
from oracle import pyref
from pointnerf_amd import config, editing, scenes
from pointnerf_amd.neural_points import NeuralPoints


@pytest.mark.parametrize("name", E.CASES)
def test_restatement_matches_the_reference_aggregator(name):
    """the bar of tests/test_oracle_golden.py for agg_small_k*.npz (2e-6: same fp32 ops); measured 0.0"""
    torch.set_num_threads(1)
    fix = np.load(E.FIXTURE)
    _, _, ref = E.reference(name)
    for key, got in (("output", ref["decoded_features"]), ("weight", ref["weight"])):
        b = fix["%s.%s" % (name, key)]
        err = np.abs(got.numpy() - b).max()
        print(name, key, "restatement - reference: %.1e" % err)
        assert got.shape == b.shape and err <= 2e-6 * max(1.0, np.abs(b).max()), (key, err)
    assert np.array_equal(ref["ray_valid"].numpy(), fix[name + ".ray_valid"])
    # the case is a test of the feature: most valid samples mix parts, and the frames move the per-sample outputs far above the bar
    opt, xyz, attrs, inp, mlp = E.reference(name)[0]
    Fg = E.gather_frames(E.case_frames(name), ref["query"]["sample_pidx"])
    mixed = ((Fg != Fg[:, :, :, :1]).flatten(-2).any(-1) & ref["neighbors"]["mask"]).any(-1)
    assert int(mixed.sum()) > int(ref["ray_valid"].sum()) // 2
    with torch.no_grad():
        ident = pyref.render(opt, dict(xyz=xyz, **attrs), mlp, inp, q=ref["query"])
    assert float((ident["decoded_features"] - ref["decoded_features"]).abs().max()) > 100 * E.BAR


@pytest.mark.parametrize("name", E.CASES)
def test_equal_frames_are_the_uniform_path(name):
    """all frames = Q: pyref.aggregate(Rw2c=Q) within 1e-6 (measured 3e-7: the batched product sums in another order)"""
    torch.set_num_threads(1)
    (opt, xyz, attrs, inp, mlp), _, ref = E.reference(name)
    Q = E.rotations()[1]
    with torch.no_grad():
        got = E.render_frames(opt, dict(xyz=xyz, **attrs), mlp, inp, Q[None].expand(xyz.shape[0], -1, -1).contiguous(), q=ref["query"])
        want = pyref.render(opt, dict(xyz=xyz, **attrs), mlp, inp, q=ref["query"], Rw2c=Q)
    err = float((got["decoded_features"] - want["decoded_features"]).abs().max())
    print(name, "all frames = Q against the uniform oracle: %.1e" % err)
    assert err <= 1e-6
    assert torch.equal(got["weight"], want["weight"])


# ------------------------------------------------------------------------------------------------- compose_parts
def _state(n, seed, rw=None):
    a = scenes.point_attributes(n, 32, seed)
    sd = {"neural_points.xyz": torch.from_numpy(scenes.chair_points(n, seed=seed))}
    sd.update({"neural_points." + k: torch.from_numpy(v) for k, v in a.items()})
    if rw is not None:
        sd["neural_points.Rw2c"] = rw
    return sd


def _mat(rot, tran):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3], m[:3, 3] = rot, tran
    return m


def test_compose_parts_restates_the_reference_loop():
    rots = E.rotations(4, seed=7).numpy()
    g = np.random.default_rng(0)
    old = torch.from_numpy(rots[3].copy())
    table = E.make_frames(50, seed=9)[0]
    parts = [(_state(60, 0), torch.from_numpy(g.random(60) < 0.5), _mat(rots[1], [0.1, -0.2, 0.3])),         # no stored frame: Rw2c = Rot
             (_state(40, 1, rw=old), None, _mat(rots[2], [0.0, 0.5, 0.0])),                                  # stored [3,3]: Rw2c_old @ Rot^T
             (_state(30, 2, rw=torch.eye(3)), torch.from_numpy(g.random(30) < 0.7), _mat(np.eye(3), [1.0, 2.0, 3.0])),   # pure translation
             (_state(50, 3, rw=table), torch.from_numpy(g.random(50) < 0.6), _mat(rots[1], [0.0, 0.0, 0.0])),  # stored per-point table
             (_state(20, 4), None, None)]                                                                     # no transform at all
    xyz, emb, color, pdir, conf, rw = editing.compose_parts(parts)
    # numpy restatement of run/editing.py:194-209
    want = {k: [] for k in ("xyz", "emb", "color", "dir", "conf", "rw")}
    for sd, inds, mat in parts:
        n = sd["neural_points.xyz"].shape[0]
        sel = np.ones(n, bool) if inds is None else inds.numpy()
        mat = np.eye(4, dtype=np.float32) if mat is None else mat
        x = sd["neural_points.xyz"].numpy()[sel]
        want["xyz"].append((np.concatenate([x, np.ones_like(x[:, :1])], -1) @ mat.T)[:, :3])
        for k, key in (("emb", "points_embeding"), ("color", "points_color"), ("dir", "points_dir"), ("conf", "points_conf")):
            want[k].append(sd["neural_points." + key].numpy()[:, sel])
        rot = mat[:3, :3]
        if "neural_points.Rw2c" not in sd:
            r = np.broadcast_to(rot, (len(x), 3, 3))
        else:
            o = sd["neural_points.Rw2c"].numpy()
            r = o[sel] @ rot.T if o.ndim == 3 else np.broadcast_to(o @ rot.T, (len(x), 3, 3))
        want["rw"].append(r)
    M = sum(len(x) for x in want["xyz"])
    assert xyz.shape == (M, 3) and emb.shape == (1, M, 32) and color.shape == (1, M, 3) and pdir.shape == (1, M, 3) and conf.shape == (1, M, 1)
    assert rw.shape == (M, 3, 3) and rw.is_contiguous()
    assert np.abs(xyz.numpy() - np.concatenate(want["xyz"], 0)).max() <= 1e-6
    assert np.abs(rw.numpy() - np.concatenate(want["rw"], 0)).max() <= 1e-6
    for got, k in ((emb, "emb"), (color, "color"), (pdir, "dir"), (conf, "conf")):
        assert np.array_equal(got.numpy(), np.concatenate(want[k], 1)), k
    # the pure translation leaves the frames at identity and only shifts the points; the untouched part is returned as stored
    n0, n1 = len(want["xyz"][0]), len(want["xyz"][1])
    n2 = len(want["xyz"][2])
    assert torch.equal(rw[n0 + n1:n0 + n1 + n2], torch.eye(3)[None].expand(n2, -1, -1))
    assert torch.equal(rw[-20:], torch.eye(3)[None].expand(20, -1, -1)) and torch.equal(xyz[-20:], parts[4][0]["neural_points.xyz"])
    # both branches of the rule occur and differ
    assert torch.allclose(rw[0], torch.from_numpy(rots[1])) and torch.allclose(rw[n0], old @ torch.from_numpy(rots[2]).T, atol=1e-6)
    with pytest.raises(ValueError):
        editing.compose_parts([(_state(10, 0), torch.ones(9, dtype=torch.bool), None)])
    with pytest.raises(ValueError):
        editing.compose_parts([])


# ------------------------------------------------------------------------------------------------- the frame table follows the points
def _cloud(n=100, seed=2, editing_entry=False):
    opt = config.lego_opt()
    npnt = NeuralPoints(32, n, opt, torch.device("cpu"))
    a = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, 32, seed).items()}
    frames = E.make_frames(n, seed=seed)[0]
    kw = dict(points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"], Rw2c=frames.clone())
    xyz = torch.from_numpy(scenes.chair_points(n, seed=seed))
    if editing_entry:
        npnt.editing_set_points(xyz, a["points_embeding"], **kw)
    else:
        npnt.set_points(xyz, a["points_embeding"], parameter=True, **kw)
    return npnt, frames


@pytest.mark.parametrize("editing_entry", [False, True])
def test_prune_and_grow_keep_frame_rows_aligned_with_points(editing_entry):
    npnt, frames = _cloud(editing_entry=editing_entry)
    if editing_entry:       # neural_points.py:470-486: nothing is wrapped, Rw2c kept as given
        assert not isinstance(npnt.Rw2c, torch.nn.Parameter) and not isinstance(npnt.xyz, torch.nn.Parameter)
    else:
        assert isinstance(npnt.Rw2c, torch.nn.Parameter) and not npnt.Rw2c.requires_grad
    assert torch.equal(npnt.Rw2c.data, frames)
    npnt.eulers = torch.arange(300, dtype=torch.float32).view(100, 3)
    keepm = npnt.points_conf.detach()[0, :, 0] >= 0.5
    xyz_before = npnt.xyz.detach().clone()
    npnt.prune(0.5)
    keep = int(keepm.sum())
    assert 0 < keep < 100 and npnt.Rw2c.shape == (keep, 3, 3) and npnt.eulers.shape == (keep, 3)
    assert torch.equal(npnt.Rw2c.detach(), frames[keepm]) and torch.equal(npnt.xyz.detach(), xyz_before[keepm])
    assert torch.equal(npnt.eulers.detach(), torch.arange(300, dtype=torch.float32).view(100, 3)[keepm])
    add = 7
    new = E.rotations(3, seed=5)[torch.arange(add) % 3]
    grow = lambda **kw: npnt.grow_points(torch.zeros(add, 3), torch.zeros(add, 32), torch.zeros(add, 3), torch.zeros(add, 3), torch.ones(add, 1), **kw)
    with pytest.raises(ValueError):          # a cloud with per-point frames needs the new points' frames
        grow()
    with pytest.raises(ValueError):
        grow(add_Rw2c=new[None], add_eulers=torch.zeros(add, 3))       # the reference's [1,add,3,3] form: wrong axis
    grow(add_Rw2c=new, add_eulers=torch.ones(add, 3))
    assert npnt.xyz.shape == (keep + add, 3) and npnt.Rw2c.shape == (keep + add, 3, 3) and npnt.eulers.shape == (keep + add, 3)
    assert torch.equal(npnt.Rw2c.detach()[:keep], frames[keepm]) and torch.equal(npnt.Rw2c.detach()[keep:], new)
    assert isinstance(npnt.Rw2c, torch.nn.Parameter) != editing_entry
    # a cloud with ONE frame ignores the per-point arguments, as before
    one, _ = _cloud()
    one.set_points(one.xyz.detach(), one.points_embeding.detach(), points_color=one.points_color.detach(), points_dir=one.points_dir.detach(),
                   points_conf=one.points_conf.detach(), parameter=True, Rw2c=E.rotations()[1].clone())
    one.grow_points(torch.zeros(add, 3), torch.zeros(add, 32), torch.zeros(add, 3), torch.zeros(add, 3), torch.ones(add, 1), add_Rw2c=new)
    one.prune(0.5)
    assert one.Rw2c.shape == (3, 3)
    with pytest.raises(ValueError):
        NeuralPoints(32, 5, config.lego_opt(), torch.device("cpu")).set_points(torch.zeros(5, 3), torch.zeros(1, 5, 32), Rw2c=torch.zeros(4, 3, 3))


def test_checkpoint_round_trip_of_the_frame_table(tmp_path):
    from pointnerf_amd.mvs_points_volumetric_model import create_model
    n = 50
    mk = lambda **kw: config.lego_train_opt(**dict(dict(gpu_ids=[], checkpoints_dir=str(tmp_path), name="run", resume_dir="", num_point=n, K=4, SR=8), **kw))
    m = create_model(mk())
    a = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, 32, 0).items()}
    frames = E.make_frames(n, seed=4)[0]
    xyz = torch.from_numpy(scenes.chair_points(n, seed=0))
    m.set_points(xyz, a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"], Rw2c=frames.clone())
    m.save_networks(7, {})
    sd = torch.load(str(tmp_path / "run" / "7_net_ray_marching.pth"))
    assert torch.equal(sd["neural_points.Rw2c"], frames)
    opt2 = mk(resume_iter=7, resume_dir=str(tmp_path / "run"), load_points=1)
    m2 = create_model(opt2)
    m2.setup(opt2)
    rw = m2.neural_points.Rw2c
    assert isinstance(rw, torch.nn.Parameter) and not rw.requires_grad and torch.equal(rw.data, frames)
    # the editing entry of the shell (run/editing.py:211): tensors as given
    m2.set_points(xyz, a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"],
                  Rw2c=frames, editing=True)
    assert m2.neural_points.Rw2c is frames and m2.neural_points.xyz is xyz
