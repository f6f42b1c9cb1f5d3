"""dev: when does each workgroup of the K-rows class launch of k_agg_forward / k_agg_backward finish?  (bench workload, configs[1])

Needs libpnerf_hip.so built with  make -C pointnerf_amd/csrc -B EXTRA_DEFS=-DPN_PHASE_TRACE  (never the shipped build): thread 0 of every
workgroup stamps the 100 MHz clock at the top of its first tile and at the end of every tile (PN_TR_SPAN, csrc/mlp_common.h); the last stamp
is the workgroup's finish time.  Idle slot-time = sum over workgroups of (last finish of the launch - own finish), as a fraction of
workgroups x (last finish - first start).  Prints one JSON object (profiles/dynamic_tiles.json keeps it)."""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from pointnerf_amd import config, _lib, dist as pdist

WGS, STEPS = 512, 4
dev = torch.device("cuda:0")
opt = config.bench_lego_opt(is_train=1)
model = bench.build_model(opt, 2_000_000, dev)
agg, npnt = model.aggregator, model.neural_points
params = [p for p in agg.parameters()] + [npnt.points_embeding, npnt.points_conf, npnt.points_dir, npnt.points_color]
lib = _lib.lib()


def read(name):
    buf = np.zeros(WGS * 4, dtype=np.uint64)
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(buf.nbytes))
    assert rc == 0, rc
    return buf.reshape(WGS, 4).astype(np.int64)


def spans(t):
    t = t[t[:, 2] > 0]
    start, end, tiles = t[:, 0], t[:, 1], t[:, 2]
    t0, t1 = start.min(), end.max()
    fin = (end - t0) * 0.01                     # us after the launch's first stamp
    launch = float(t1 - t0) * 0.01
    idle = float((t1 - end).sum()) * 0.01
    return {"workgroups": int(len(t)), "launch_us": round(launch, 1), "finish_us_median": round(float(np.median(fin)), 1),
            "finish_us_p10": round(float(np.percentile(fin, 10)), 1), "finish_us_p90": round(float(np.percentile(fin, 90)), 1),
            "finish_us_min": round(float(fin.min()), 1), "finish_us_max": round(float(fin.max()), 1),
            "first_stamp_spread_us": round(float(start.max() - t0) * 0.01, 1),
            "idle_slot_us_per_workgroup": round(idle / len(t), 1), "idle_slot_fraction": round(idle / (len(t) * launch), 5),
            "tiles_per_workgroup_min_median_max": [int(tiles.min()), int(np.median(tiles)), int(tiles.max())], "tiles": int(tiles.sum())}


res = {"forward": [], "backward": []}
for i in range(2 + STEPS):
    for p in params:
        p.grad = None
    inp = bench.step_inputs(i, 0, 1, 65536, dev)
    out = model(**inp)
    loss = pdist.hot_path_loss(opt, out, inp["gt_image"])
    loss.backward()
    torch.cuda.synchronize()
    if i >= 2:                                  # (the stamps are the last step's: read them step by step)
        res["forward"].append(spans(read("pnerf_debug_span_fwd")))
        res["backward"].append(spans(read("pnerf_debug_span_bwd")))
print(json.dumps(res, indent=1))
