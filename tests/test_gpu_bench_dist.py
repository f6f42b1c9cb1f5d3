"""bench.py end to end on the GPU: the single-process JSON contract, and the multi-process path (2 ranks sharing the
one GPU of the test box over gloo, since RCCL refuses two ranks on one device) -- same code path the driver launches
with --nproc-per-node N over RCCL."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json(out):
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.decode()[-2000:]
    return json.loads(lines[0])


def test_bench_json_contract_single_gpu():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--rays", "8192",
                                   "--points", "300000", "--cpu-rays", "64", "--full"], cwd=ROOT, timeout=900)
    d = _last_json(out)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["unit"] == "rays/s" and d["value"] > 0 and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["config"]["final_loss"] == d["config"]["final_loss"] and abs(d["config"]["final_loss"]) < 1e3      # finite: a NaN step is not a step
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["peak"] > 0 and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    # the headline line carries the fp32-class weight-gradient variant of the same step (--wgrad-planes 2) next to the shipped arithmetic
    v = d["config"]["fp32_class_variant"]
    assert d["config"]["wgrad_planes"] == 1 and v["ms_per_step"] > 0 and v["value"] > 0 and abs(v["final_loss"]) < 1e3
    assert d["scaling"] == "weak" and d["config"]["global_batch_rays"] == 8192        # (N = 1: the two readings coincide)
    # ... and the other priced variants of the same step: f16 cross terms everywhere (the round-5 arithmetic), e4m3 cross terms in the training forward
    # too, and the route the reference's unmodified shell takes (compacted outputs, ATen losses, two torch.optim.Adam)
    for name in ("f16_cross_terms_variant", "e4m3_forward_variant", "reference_shell_variant"):
        vv = d["config"][name]
        assert vv["ms_per_step"] > 0 and vv["value"] > 0 and abs(vv["final_loss"]) < 1e3, name
    hb = d["roofline_hbm"]["agg_backward"]
    assert hb["survey_algorithmic_bytes_per_step"] > 0 and d["cpu_baseline"].get("note") or d["cpu_baseline"]["kind"] == "reference"
    # and the mode can be timed on its own
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--rays", "8192",
                                   "--points", "300000", "--cpu-rays", "0", "--wgrad-planes", "2", "--full"], cwd=ROOT, timeout=900)
    d2 = _last_json(out)
    assert d2["config"]["wgrad_planes"] == 2 and "fp32_class_variant" not in d2["config"] and "3 products" in d2["dtype"]
    assert abs(d2["config"]["final_loss"] - d["config"]["final_loss"]) <= 1e-4 * max(1.0, abs(d["config"]["final_loss"]))


def test_plain_bench_times_only_the_headline_and_dumps_its_last_step(tmp_path):
    """without --full the line carries the headline and nothing that needs runs of its own; --dump-outputs writes the last timed step's
    results (float32 / float64, 64 MB at most), and two runs with the same arguments compute the same from the same inputs"""
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rays", "8192", "--points", "300000"]
    runs = []
    for tag in ("a", "b"):
        d = _last_json(subprocess.check_output(base + ["--dump-outputs", str(tmp_path / tag)], cwd=ROOT, timeout=900))
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "rays/s"
        for k in ("roofline", "roofline_mfma", "roofline_hbm", "kernels", "ms_outside_library_kernels", "cpu_baseline"):
            assert k not in d, k
        for k in ("ms_step_cold_grid", "ms_step_without_optimizer", "f16_cross_terms_variant", "e4m3_forward_variant", "reference_shell_variant",
                  "fp32_class_variant"):
            assert k not in d["config"], k
        files = sorted(os.listdir(str(tmp_path / tag)))
        arrays = {f[:-4]: np.load(str(tmp_path / tag / f)) for f in files}
        assert all(f.endswith(".npy") for f in files) and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(os.path.getsize(str(tmp_path / tag / f)) for f in files) <= 64 << 20
        for k in ("loss", "coarse_raycolor", "ray_mask", "points_embeding", "points_embeding_grad", "mlp.block1.0.weight", "mlp_grad.block1.0.weight"):
            assert k in arrays, k
        assert all(np.isfinite(a).all() for a in arrays.values())
        assert float(arrays["loss"][0]) == np.float32(d["config"]["dump"]["loss_of_dumped_step"])
        assert np.isfinite(d["config"]["final_loss"]) and d["config"]["dump"]["ms_state_reset_before_last_step"] >= 0
        assert arrays["coarse_raycolor"].shape == (int(arrays["ray_mask"].sum()), 3) and arrays["points_embeding"].shape == (65536, 32)
        runs.append(arrays)
    a, b = runs
    assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape for k in a)
    # the last step starts from the seeded initial state: its forward is bit-reproducible, gradients and update differ by the order of
    # the backward's atomic additions only
    assert np.array_equal(a["ray_mask"], b["ray_mask"]) and np.array_equal(a["coarse_raycolor"], b["coarse_raycolor"])
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-6 * abs(float(a["loss"][0]))
    for k in a:
        scale = max(float(np.abs(a[k]).max()), 1e-30)
        assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= 1e-4 * scale, (k, float(np.abs(a[k].astype(np.float64) - b[k]).max()), scale)


def test_bench_refuses_a_gpu_count_it_was_not_launched_with():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], cwd=ROOT, capture_output=True, timeout=300)
    assert r.returncode != 0 and b"WORLD_SIZE=1" in r.stderr


def test_touched_flags_kernel_equals_the_torch_form():
    import torch
    from pointnerf_amd import dist as pdist
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    for n, shape, frac_empty in ((5000, (300, 8), 0.3), (70, (4, 16, 8), 0.0), (1, (9,), 1.0), (1000, (0, 8), 0.0)):
        pidx = torch.randint(0, n, shape, generator=g, dtype=torch.int32)
        if frac_empty:
            pidx[torch.rand(shape, generator=g) < frac_empty] = -1
        want = pdist.touched_flags(pidx, n)                       # CPU tensors: the torch form
        got = pdist.touched_flags(pidx.to(dev), n)                # device int32 table: pnerf_touched_flags
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (n, shape)
    assert pdist.touched_flags(torch.zeros(4, 8, dtype=torch.int32, device=dev), 0).numel() == 0


def _free_port():
    """a port nobody holds right now (fixed port formulas of neighbouring tests can collide)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _two_ranks(extra, port_off):
    env = dict(os.environ, PNERF_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--rays", "4096", "--points", "300000", "--cpu-rays", "0"] + extra
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, timeout=900, stderr=subprocess.STDOUT)
    assert b"rccl_selftest: ok" in out and b"world=2" in out, out.decode()[-2000:]        # every collective form of the step ran once before the timing
    d = _last_json(out)
    c = d["config"]
    assert len(c["ms_allreduce_exposed_by_rank"]) == 2 and all(t >= 0 for t in c["ms_allreduce_exposed_by_rank"])
    # every rank applied the same summed gradients: the replicas' parameters are bitwise identical (incl. points_conf[0], which collects
    # the zero-one regulariser's empty-slot terms: ADVICE round 2 on the sparse exchange)
    assert c["replica_param_checksum_spread"] == 0.0, c["replica_param_checksum_spread"]
    return d


def test_bench_two_ranks_on_one_gpu():
    d = _two_ranks([], 0)
    # N > 1 defaults to BASELINE.json configs[2] as SURVEY 8d defines it: ONE global batch of --rays rays split contiguously over the ranks
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["global_batch_rays"] == 4096 and d["config"]["rays_per_gpu_per_step"] == 2048 and "configs[2]" in d["config"]["workload"]
    assert "cpu_baseline" not in d                      # rank 0 at N=1 only
    w = _two_ranks(["--weak"], 1)                       # the optional weak-scaling variant: --rays rays per GPU
    assert w["scaling"] == "weak" and w["config"]["global_batch_rays"] == 8192 and w["config"]["rays_per_gpu_per_step"] == 4096
    # the point-gradient all-reduce issued on a side stream behind the library's "point gradients ready" event (overlapping the
    # weight-gradient GEMMs; the default) gives the same training trajectory as the all-reduce after the whole backward
    n = _two_ranks(["--no-overlap-comm"], 3)
    assert abs(n["config"]["final_loss"] - d["config"]["final_loss"]) <= 1e-6 * max(1.0, abs(d["config"]["final_loss"]))
    # ZeRO-1 sharding of the point-parameter Adam is the same update: the loss after 3 steps agrees to summation order
    z = _two_ranks(["--zero1"], 7)
    assert abs(z["config"]["final_loss"] - d["config"]["final_loss"]) <= 1e-5 * max(1.0, abs(d["config"]["final_loss"]))
    assert d["config"]["point_grad_exchange"].startswith("dense") and z["config"]["point_grad_exchange"].startswith("zero1")
    # the touched-row exchange (the default from 6 M points) is the same sum
    s = _two_ranks(["--point-grads", "sparse"], 11)
    assert s["config"]["point_grad_exchange"].startswith("sparse")
    assert abs(s["config"]["final_loss"] - d["config"]["final_loss"]) <= 1e-5 * max(1.0, abs(d["config"]["final_loss"]))


def test_point_gradients_reach_autograd_as_views_of_one_bucket():
    """what the one-collective early all-reduce relies on: after loss.backward() the .grad of the embedding / dir / colour parameters
    ARE the renderer's views (not autograd clones), contiguous at the head of the bucket"""
    import torch
    import bench
    from pointnerf_amd import config
    from pointnerf_amd.fused import FusedRender
    dev = torch.device("cuda:0")
    opt = config.bench_lego_opt(is_train=1)
    model = bench.build_model(opt, 200_000, dev)
    inp = bench.step_inputs(0, 0, 1, 2048, dev)
    out = model(**inp)
    bench.loss_fn(opt, out, inp, 1).backward()
    npnt = model.neural_points
    bucket, head, ptrs = FusedRender.point_grad_bucket
    got = [npnt.points_embeding.grad, npnt.points_dir.grad, npnt.points_color.grad]
    assert [g.data_ptr() for g in got] == list(ptrs)
    assert got[0].data_ptr() == bucket.data_ptr() and head >= sum(g.numel() for g in got)
    assert float(bucket[:head].abs().sum()) > 0


def test_measured_matrix_pipe_ceiling_is_sane():
    """ops.mfma_rate_tflops (pnerf_debug_mfma_rate): the f16 matrix pipe's sustained rate, timed on this box -- between a fifth of the nominal 2.5 PFLOP/s and
    the nominal figure, and not HIGHER with operands that toggle than with one constant (measured on MI355X: 1.70 vs 2.33 PFLOP/s)."""
    from pointnerf_amd import ops
    ops.mfma_rate_tflops(1, ms_target=30.0)                  # (the first call of a cold process also pays the clock's way up from idle)
    const, rnd = ops.mfma_rate_tflops(1, ms_target=30.0), ops.mfma_rate_tflops(2, ms_target=30.0)
    print("matrix pipe, register-resident f16 MFMA: constant operands %.0f TFLOP/s, pseudo-random operands %.0f TFLOP/s" % (const, rnd))
    # sanity only (this is a measurement aid, not a parity claim): both inside physical bounds, toggling operands not clearly FASTER than constants
    assert 500.0 < rnd < 2700.0 and 500.0 < const < 2700.0 and rnd <= 1.15 * const, (const, rnd)


def test_collective_selftest_on_rccl_with_one_rank():
    """RCCL refuses two ranks on one device, so the 2-rank tests above run over gloo; this runs bench.rccl_selftest on the REAL backend ("nccl" = RCCL)
    with a world of one: the library loads, a communicator forms, and every collective form the step uses is a valid call on that backend
    (all_reduce, all_gather_into_tensor, the in-place reduce_scatter_tensor, the side-stream all-reduce of a bucket head behind an event with
    record_stream) -- gloo has no reduce_scatter and takes list-form all_gather, so those two forms run nowhere else before the 8-GPU node."""
    code = (
        "import os, sys, torch\n"
        "sys.path.insert(0, %r)\n"
        "import socket\n"
        "sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')\n"
        "import bench\n"
        "with bench.Watchdog('init_process_group', 120, 0, 1):\n"
        "    torch.distributed.init_process_group(backend='nccl')\n"
        "torch.cuda.set_device(0)\n"
        "dev = torch.device('cuda', 0)\n"
        "with bench.Watchdog('selftest', 90, 0, 1):\n"
        "    print(bench.rccl_selftest(dev, 0, 1))\n"
        "torch.distributed.destroy_process_group()\n"
        "print('rccl one-rank ok')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "rccl one-rank ok" in r.stdout and "ok backend=nccl world=1" in r.stdout, (r.returncode, r.stdout[-800:], r.stderr[-1500:])


def test_every_collective_of_the_step_on_rccl_with_one_rank():
    """bench.py --force-collectives: a one-rank RCCL group with every collective of the step executed (as identities) -- the overlapped one-bucket
    all-reduce on the side stream behind the library's event, the after-backward form, ZeRO-1's in-place reduce-scatter / all-gather and the sparse
    touched-row exchange with all_gather_into_tensor: the calls the 8-GPU run makes, on the backend it makes them on.  Being identities, each form
    must reproduce the plain single-GPU step's loss."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--rays", "8192", "--points", "300000", "--cpu-rays", "0",
            "--no-fp32-class-variant"]
    plain = _last_json(subprocess.check_output(base, cwd=ROOT, timeout=900))
    for extra, label in (([], "dense all-reduce"), (["--no-overlap-comm"], "dense all-reduce"), (["--zero1"], "zero1"), (["--point-grads", "sparse"], "sparse")):
        r = subprocess.run(base + ["--force-collectives"] + extra, cwd=ROOT, capture_output=True, timeout=900)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"rccl_selftest: ok  backend=nccl world=1" in r.stderr, r.stderr.decode()[-1500:]
        d = _last_json(r.stdout)
        c = d["config"]
        assert c["point_grad_exchange"].startswith(label) and c["collective_selftest"].startswith("ok backend=nccl"), c["point_grad_exchange"]
        assert c["replica_param_checksum_spread"] == 0.0 and len(c["ms_allreduce_exposed_by_rank"]) == 1
        assert abs(c["final_loss"] - plain["config"]["final_loss"]) <= 1e-5 * max(1.0, abs(plain["config"]["final_loss"])), (extra, c["final_loss"], plain["config"]["final_loss"])
