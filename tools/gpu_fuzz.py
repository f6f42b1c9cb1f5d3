"""dev: random small configurations (K, SR, P, cloud size, view) through the parity checks of tests/test_gpu_query.py / test_gpu_render.py /
test_gpu_backward.py -- a net for rare shapes the fixed test matrix does not hit"""
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import test_gpu_query as TQ, test_gpu_backward as TB
from pointnerf_amd import config, scenes
from oracle import pyref

rng = random.Random(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 20
bad = 0
for it in range(n_cases):
    K = rng.choice([1, 2, 3, 4, 5, 6, 8, 8, 8, 12, 16])
    SR = rng.choice([4, 8, 17, 24, 40, 64, 70, 128])
    P = rng.choice([6, 9, 12, 20, 26, 32])
    n = rng.choice([1500, 3000, 6000, 12000])           # (small clouds: one LeakyReLU-kink row is already > 0.2 % of the per-point elements)
    size = rng.choice([1, 3, 6, 9, 12])
    radius = rng.choice([0.03, 0.06, 0.1])
    seed = rng.randrange(100)
    kw = dict(K=K, SR=SR, P=P, max_o=50000, ranges=[-0.3, -0.3, -0.3, 0.3, 0.3, 0.3])
    if rng.random() < 0.3:
        kw["vsize"] = rng.choice([[0.008, 0.008, 0.008], [0.02, 0.02, 0.02], [0.004, 0.006, 0.0045]])      # (not vsize[2] = 0.005: 2 x vsize[2] would equal the depth step, the knife edge of ray_dist's "d > 2 vsize" rule)
    desc = dict(K=K, SR=SR, P=P, n=n, size=size, radius=radius, seed=seed, **{k: v for k, v in kw.items() if k == "vsize"})
    try:
        opt = config.lego_opt(**kw)
        xyz = torch.from_numpy(scenes.chair_points(n, seed=seed, radius=radius))
        attrs = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, 32, seed).items()}
        inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=rng.uniform(0, 360), x0=400 - size // 2, y0=400 - size // 2, size=size))
        q = pyref.query(opt, xyz, inp)
        TQ._assert_same(q, *TQ._native_op(opt, xyz, inp, q["hp"]))
        if int((q["sample_pidx"] >= 0).sum()) == 0:
            print("ok (query only, no hits)", desc); continue
        mlp = pyref.init_mlp_params(opt, seed=seed, bias_scale=0.1)
        TB._run(opt, xyz, attrs, inp, mlp)
        print("ok", desc)
    except Exception as e:
        bad += 1
        print("FAIL", desc, repr(e)[:300])
print("cases", n_cases, "failures", bad)
