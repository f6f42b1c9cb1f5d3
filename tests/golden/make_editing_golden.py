"""Generate tests/golden/editing_frames.npz from the REFERENCE's own PointAggregator run with one Rw2c frame per gathered neighbor
([1,R,SR,K,3,3]: models/aggregators/point_aggregators.py:492-496,506,526,566), on the CPU, for the seeded cases of tests/editing_case.py
(run where the reference exists; the tests only read the committed .npz, which holds numeric arrays only).

    python tests/golden/make_editing_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PointAggregator, ref_opt, pyref, build_case      # noqa: E402  (imports the reference)
import editing_case as E                                                  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    fix = {}
    for name in E.CASES:
        opt, xyz, attrs, inp, mlp = build_case(name)
        frames = E.case_frames(name)
        with torch.no_grad():
            q = pyref.query(opt, xyz, inp)
            nb = pyref.gather_neighbors(dict(xyz=xyz, **attrs), q["sample_pidx"], inp["camrotc2w"][0], inp["campos"][0])
            agg = PointAggregator(ref_opt(opt))
            agg.load_state_dict(mlp, strict=True)
            Fg = E.gather_frames(frames, q["sample_pidx"])
            out, ray_valid, weight, _ = agg(nb["color"], Fg, nb["dir"], nb["conf"], nb["emb"], nb["xyz_pers"], nb["xyz"], nb["mask"],
                                            q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"], q["hp"]["vsize"], 0)
            ident, _, _, _ = agg(nb["color"], torch.eye(3), nb["dir"], nb["conf"], nb["emb"], nb["xyz_pers"], nb["xyz"], nb["mask"],
                                 q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"], q["hp"]["vsize"], 0)
        fix[name + ".output"], fix[name + ".ray_valid"], fix[name + ".weight"] = out.numpy(), ray_valid.numpy(), weight.numpy()
        mine = E.aggregate_frames(opt, mlp, nb, q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"], Fg)[0]
        mixed = int(((Fg != Fg[:, :, :, :1]).flatten(-2).any(-1) & nb["mask"]).any(-1).sum())
        print(name, "valid samples", int(ray_valid.sum()), "rows", int(nb["mask"].sum()), "samples that mix parts", mixed,
              "| restatement - reference %.1e" % float((mine - out).abs().max()),
              "| frames move sigma / rgb by %.2f / %.2f" % (float((out - ident)[..., 0].abs().max()), float((out - ident)[..., 1:].abs().max())),
              "| valid samples with an empty slot 0:", int((ray_valid & ~nb["mask"][..., 0]).sum()))
    np.savez_compressed(os.path.join(HERE, "editing_frames.npz"), **fix)


if __name__ == "__main__":
    main()
