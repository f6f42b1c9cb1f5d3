"""Point attribute maps, picking and lifting (include/pnerf.h pnerf_ray_attributes / pnerf_lift_to_points, pointnerf_amd/point_maps.py,
DESIGN.md 4.8): the seeded inputs, the float64 numpy restatements and the checks that tests/test_pointmaps_emu.py (host emulator) and
tests/test_gpu_pointmaps.py (device) share.

With p = sample_pidx[r,s,k] and g[r,s,k] = blend_w[r,s] * weight[r,s,k] where 0 <= p < n_points (else 0):
  attr_sum[r,c] = sum_{s,k} g attr[p,c];   top_flat = the lowest flat index among the maxima of g[r], top_point / top_contrib = p / g there,
  -1 / -1 / 0 where no g is > 0;   point_sum[p,c] += g m[r] values[r,c],  point_mass[p] += g m[r].

Kernel cases: R = 37 rays, n_points = 500, synthetic.  Random -1 slots, entries with pidx == n_points (the tables carry one extra row of NaN and
n_points is passed as is: a missing range guard shows as NaN, not as a fault), whole samples with blend_w = 0, a hit ray with all blend_w = 0,
missed rays whose rows are NaN, and exact ties of the maximum in different samples and (where SR*K > 64) in different 64-entry chunks.

Bars, u = 2^-24, from the worst-case error of an fp32 sum of n terms in any order (n - 1 roundings of partial sums, each at most u times the
sum of absolute values) plus the roundings of a term:
  attr_sum   |got - f64| <= (SR*K + 2) u A,  A = the float64 sum of |g attr| over the ray, g in float64 the exact product of the fp32 inputs
             (a term carries two roundings, the sum SR*K - 1); a sequential numpy fp32 restatement is held to the same bar;
  top_*      bit for bit numpy's float32 product and its first argmax (a single multiply leaves nothing to round differently);
  lift       per point and column |got - f64| <= (n_p + 3) u A_p, n_p the contributing entries that address p (a term carries three
             roundings); points nothing addresses stay exactly 0; a second call into the same accumulators doubles it at 2 n_p;
  adjoint    |<y, A x> - <A^T y, x>| formed in float64 from the device results, within the sum of the two bounds."""
import ctypes

import numpy as np
import pytest
import torch

import cutoff_case as C
import editing_case as E

U = 2.0 ** -24
BAR = C.BAR
NEAR = 1e-3
R, N_POINTS = 37, 500
SRS, KS = (1, 16, 65, 128), (1, 3, 8, 12, 16)
CS = (0, 1, 3, 4, 5, 32, 33, 64, 70)
LIFT_CS = (0, 1, 3, 8)
EMU_SHAPES = [(1, 1), (1, 16), (16, 3), (16, 8), (65, 1), (65, 12)]      # the smallest sizes: SR*K below, across and a few times 64
ALL_ZERO_RAY, TIE_RAYS = 5, (7, 8, 9)


# ------------------------------------------------------------------------------------------------- inputs
def kernel_inputs(SR, K, seed=0):
    """dict of numpy arrays: blend_w [R,SR] f32, weight [R,SR,K] f32, pidx [R,SR,K] i32, hit [R] i32 (what the kernel is handed: NaN rows on the
    rays that missed) and ``ties``: {ray: (flat index that must win, the other one)}"""
    rng = np.random.default_rng(4000 + 100 * SR + K + seed)
    n = SR * K
    pidx = rng.integers(0, N_POINTS, size=(R, SR, K)).astype(np.int32)
    kind = rng.random((R, SR, K))
    pidx[kind < 0.30] = -1
    pidx[kind > 0.97] = N_POINTS                                              # the guard row
    weight = rng.uniform(0.05, 1.0, size=(R, SR, K)).astype(np.float32)
    bw = rng.uniform(0.01, 0.2, size=(R, SR)).astype(np.float32)
    bw[rng.random((R, SR)) < 0.3] = 0.0                                       # whole samples without a blend weight
    hit = (rng.random(R) > 0.15).astype(np.int32)
    hit[[ALL_ZERO_RAY, *TIE_RAYS]] = 1
    hit[[3, 20]] = 0
    bw[ALL_ZERO_RAY] = 0.0
    ties = {}
    if n > 1:
        for i, r in enumerate(TIE_RAYS):
            e1 = (3 * i + 1) % n
            e2 = (e1 + 64 + 5 * i) if n > 80 else n - 1                       # another 64-entry chunk where there is one
            if SR > 1 and e2 // K == e1 // K:
                e2 = (e1 // K + 1) * K + (e2 % K)                             # ... and another sample
            e2 = min(e2, n - 1)
            if e2 == e1:
                continue
            for e in (e1, e2):
                bw[r, e // K] = 0.5
                weight[r, e // K] = np.minimum(weight[r, e // K], np.float32(0.9))
            for e in (e1, e2):
                weight[r, e // K, e % K] = 1.0                                # g = 0.5 exactly, above every other entry (<= 0.45)
            pidx[r, e1 // K, e1 % K], pidx[r, e2 // K, e2 % K] = 11 + i, 211 + i
            ties[r] = (e1, e2)
    miss = hit == 0
    bw[miss] = np.nan
    weight[miss] = np.nan
    pidx[miss] = 2 ** 30                                                      # rows that must not be read
    return dict(blend_w=bw, weight=weight, pidx=pidx, hit=hit, ties=ties, SR=SR, K=K)


def table(Cn, seed=0, rows=N_POINTS):
    """[rows + 1, C] float32 in [-1, 1] with the guard row of NaN"""
    rng = np.random.default_rng(900 + Cn + seed)
    t = rng.uniform(-1, 1, size=(rows + 1, Cn)).astype(np.float32)
    t[rows] = np.nan
    return t


# ------------------------------------------------------------------------------------------------- restatements
def entries(bw, w, pidx, hit, n_points):
    """(valid [R,n] bool, g32 [R,n] float32 -- numpy's single fp32 product --, g64 [R,n] the exact product, p [R,n] clipped for indexing)"""
    Rr, SR, K = w.shape
    hitb = np.asarray(hit) > 0
    valid = (pidx >= 0) & (pidx < n_points) & hitb[:, None, None]
    bws = np.where(hitb[:, None], bw, np.float32(0))
    ws = np.where(valid, w, np.float32(0))
    g32 = np.where(valid, bws[:, :, None].astype(np.float32) * ws.astype(np.float32), np.float32(0)).astype(np.float32)
    g64 = np.where(valid, bws[:, :, None].astype(np.float64) * ws.astype(np.float64), 0.0)
    p = np.where(valid, pidx, 0)
    return valid.reshape(Rr, -1), g32.reshape(Rr, -1), g64.reshape(Rr, -1), p.reshape(Rr, -1)


def pick(g32, pidx_flat):
    idx = g32.argmax(axis=1)                                                  # numpy: the first among the maxima
    rows = np.arange(g32.shape[0])
    mx = g32[rows, idx]
    none = ~(mx > 0)
    return (np.where(none, -1, pidx_flat[rows, idx]).astype(np.int32), np.where(none, -1, idx).astype(np.int32),
            np.where(none, np.float32(0), mx).astype(np.float32))


def attr_sums(g64, p, attr):
    """(float64 sum [R,C], A = float64 sum of absolute values [R,C])"""
    t = g64[:, :, None] * attr.astype(np.float64)[p]
    t = np.where(g64[:, :, None] != 0, t, 0.0)
    return t.sum(1), np.abs(t).sum(1)


def attr_sums_fp32_sequential(g32, p, attr):
    t = np.where(g32[:, :, None] != 0, g32[:, :, None] * attr[p], np.float32(0)).astype(np.float32)
    return np.cumsum(t, axis=1, dtype=np.float32)[:, -1]


def lift_sums(valid, g64, p, m, values, n_rows):
    """float64 (mass [n_rows], A_mass, sums [n_rows,C], A_sums, n_p [n_rows]) of one lifting"""
    m64 = np.ones(g64.shape[0]) if m is None else m.astype(np.float64)
    c = g64 * m64[:, None]
    on = valid & (c != 0)
    pf, cf = p[on], c[on]
    n_p = np.bincount(pf, minlength=n_rows)
    mass, a_mass = np.bincount(pf, weights=cf, minlength=n_rows), np.bincount(pf, weights=np.abs(cf), minlength=n_rows)
    Cn = 0 if values is None else values.shape[1]
    sums, a_sums = np.zeros((n_rows, Cn)), np.zeros((n_rows, Cn))
    rr = np.broadcast_to(np.arange(g64.shape[0])[:, None], g64.shape)[on]
    for col in range(Cn):
        t = cf * values[rr, col].astype(np.float64)
        sums[:, col], a_sums[:, col] = np.bincount(pf, weights=t, minlength=n_rows), np.bincount(pf, weights=np.abs(t), minlength=n_rows)
    return mass, a_mass, sums, a_sums, n_p


# ------------------------------------------------------------------------------------------------- 1. the kernels on synthetic arrays
def _dev_inputs(x, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(x["blend_w"]), t(x["weight"]), t(x["pidx"]), t(x["hit"])


def check_ray_attributes(SR, K, dev, cs=CS):
    from pointnerf_amd import ops
    x = kernel_inputs(SR, K)
    ins = _dev_inputs(x, dev)
    hitb = x["hit"] > 0
    assert 0 < (~hitb).sum() < R
    valid, g32, g64, p = entries(x["blend_w"], x["weight"], x["pidx"], x["hit"], N_POINTS)
    want_point, want_flat, want_contrib = pick(g32, x["pidx"].reshape(R, -1))
    assert want_flat[ALL_ZERO_RAY] == -1 and (want_flat[~hitb] == -1).all()
    for r, (e1, e2) in x["ties"].items():
        assert e1 < e2 and g32[r, e1] == g32[r, e2] == np.float32(0.5) and want_flat[r] == e1, (r, e1, e2)
        assert SR == 1 or e1 // K != e2 // K
        assert SR * K <= 80 or e1 // 64 != e2 // 64
    worst = 0.0
    for Cn in cs:
        attr = table(Cn)
        a_dev = torch.from_numpy(attr).to(dev) if Cn else None
        got = {k: v.cpu().numpy() for k, v in ops.ray_attributes(a_dev, *ins, n_points=N_POINTS).items()}
        again = {k: v.cpu().numpy() for k, v in ops.ray_attributes(a_dev, *ins, n_points=N_POINTS).items()}
        assert got["attr_sum"].shape == (R, Cn) and got["attr_sum"].dtype == np.float32
        for k in ("attr_sum", "top_point", "top_flat", "top_contrib"):
            assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), ("two calls", Cn, k)
        assert np.array_equal(got["top_point"], want_point) and np.array_equal(got["top_flat"], want_flat), (SR, K, Cn)
        assert np.array_equal(got["top_contrib"].view(np.int32), want_contrib.view(np.int32)), (SR, K, Cn)
        if Cn == 0:
            continue
        ref, A = attr_sums(g64, p, attr)
        bound = (SR * K + 2) * U * A
        err = np.abs(got["attr_sum"].astype(np.float64) - ref)
        assert np.isfinite(got["attr_sum"]).all(), "a NaN: the guard row or a missed ray's row was read"
        assert (got["attr_sum"][~hitb] == 0).all() and (got["attr_sum"][ALL_ZERO_RAY] == 0).all()
        seq = np.abs(attr_sums_fp32_sequential(g32, p, attr).astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        print("SR %d K %d C %d: attr_sum error / bound %.3f (sequential fp32 numpy %.3f)"
              % (SR, K, Cn, (err / np.maximum(bound, 1e-300)).max(), (seq / np.maximum(bound, 1e-300)).max()))
        assert (seq <= bound).all(), ("the bar itself", SR, K, Cn)
        assert (err <= bound).all(), (SR, K, Cn, float((err - bound).max()))
    return worst


def check_lift(SR, K, dev, cs=LIFT_CS):
    from pointnerf_amd import ops
    x = kernel_inputs(SR, K)
    ins = _dev_inputs(x, dev)
    valid, g32, g64, p = entries(x["blend_w"], x["weight"], x["pidx"], x["hit"], N_POINTS)
    rng = np.random.default_rng(77 + SR + K)
    for Cn in cs:
        for with_factor in (False, True):
            values = rng.uniform(-1, 1, size=(R, Cn)).astype(np.float32) if Cn else None
            m = None
            if with_factor:
                m = rng.uniform(0.0, 1.0, size=R).astype(np.float32)
                m[rng.random(R) < 0.25] = 0.0
            if values is not None:
                values[x["hit"] == 0] = np.nan                               # a missed ray's values are not read either
            mass, a_mass, sums, a_sums, n_p = lift_sums(valid, g64, p, m, None if values is None else np.nan_to_num(values), N_POINTS + 1)
            assert n_p[N_POINTS] == 0
            buf_s = torch.zeros(N_POINTS + 1, Cn, dtype=torch.float32, device=dev)      # one row more than the call is told of
            buf_m = torch.zeros(N_POINTS + 1, dtype=torch.float32, device=dev)
            v_dev = None if values is None else torch.from_numpy(values).to(dev)
            m_dev = None if m is None else torch.from_numpy(m).to(dev)
            out = (buf_s[:N_POINTS], buf_m[:N_POINTS])
            for calls in (1, 2):
                ret = ops.lift_to_points(v_dev, m_dev, *ins, N_POINTS, out=out)
                assert ret[0].data_ptr() == buf_s.data_ptr() and ret[1].data_ptr() == buf_m.data_ptr()
                gs, gm = buf_s.cpu().numpy().astype(np.float64), buf_m.cpu().numpy().astype(np.float64)
                assert np.isfinite(gs).all() and np.isfinite(gm).all()
                assert (gm[n_p == 0] == 0).all() and (gs[n_p == 0] == 0).all(), "a point nothing addresses was written"
                em, es = np.abs(gm - calls * mass), np.abs(gs - calls * sums)
                bm, bs = (calls * n_p + 3) * U * calls * a_mass, (calls * n_p + 3)[:, None] * U * calls * a_sums
                assert (em <= bm).all() and (es <= bs).all(), (SR, K, Cn, with_factor, calls)
            if Cn == cs[-1] and with_factor:
                print("SR %d K %d: lift mass error / bound %.3f, n_p up to %d" % (SR, K, (em / np.maximum(bm, 1e-300)).max(), n_p.max()))
    fresh = ops.lift_to_points(None, None, *ins, N_POINTS)                      # out=None: zeroed accumulators of the op's own
    assert tuple(fresh[0].shape) == (N_POINTS, 0) and tuple(fresh[1].shape) == (N_POINTS,) and float(fresh[1].sum()) > 0


def check_adjoint(SR, K, dev):
    from pointnerf_amd import ops
    x = kernel_inputs(SR, K)
    ins = _dev_inputs(x, dev)
    valid, g32, g64, p = entries(x["blend_w"], x["weight"], x["pidx"], x["hit"], N_POINTS)
    rng = np.random.default_rng(5 + SR + K)
    xt, y = table(3, seed=50), rng.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    Ax = ops.ray_attributes(torch.from_numpy(xt).to(dev), *ins, n_points=N_POINTS)["attr_sum"].cpu().numpy().astype(np.float64)
    ATy = ops.lift_to_points(torch.from_numpy(y).to(dev), None, *ins, N_POINTS)[0].cpu().numpy().astype(np.float64)
    lhs, rhs = float((y.astype(np.float64) * Ax).sum()), float((ATy * xt[:N_POINTS].astype(np.float64)).sum())
    _, A = attr_sums(g64, p, xt)
    _, _, _, a_sums, n_p = lift_sums(valid, g64, p, None, y, N_POINTS)
    bound = float((np.abs(y) * (SR * K + 2) * U * A).sum() + (np.abs(xt[:N_POINTS]) * (n_p + 3)[:, None] * U * a_sums).sum())
    print("SR %d K %d: <y, Ax> %.9g, <A^T y, x> %.9g, difference %.3g, bound %.3g" % (SR, K, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def check_entry_refusals(dev):
    """by return code: caps -> PNERF_E_UNSUP; nulls, K = 0 / 17, SR = 0, R < 0, n_points = 0, C < 0 -> PNERF_E_INVAL; R = 0 -> 0"""
    from pointnerf_amd import _lib as L, ops
    x = kernel_inputs(16, 8)
    bw, w, pidx, hit = _dev_inputs(x, dev)
    attr = torch.from_numpy(table(3)).to(dev)
    asum = torch.empty(R, 3, device=dev)
    tp, tf = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    tc = torch.empty(R, device=dev)
    P, lib = ops._ptr, L.lib()

    def attrs(a=attr, n=N_POINTS, Cn=3, ins=(bw, w, pidx, hit), Rr=R, SR=16, K=8, outs=(asum, tp, tf, tc)):
        return lib.pnerf_ray_attributes(P(a), n, Cn, *[P(t) for t in ins], Rr, SR, K, *[P(t) for t in outs], ops._stream())
    assert attrs() == 0
    assert attrs(Cn=257) == -4 and attrs(Cn=-1) == -1
    assert attrs(K=0) == -1 and attrs(K=17) == -1 and attrs(SR=0) == -1 and attrs(Rr=-1) == -1 and attrs(n=0) == -1
    assert attrs(a=None) == -1 and attrs(outs=(None, tp, tf, tc)) == -1
    for i in range(4):
        assert attrs(ins=tuple(None if j == i else t for j, t in enumerate((bw, w, pidx, hit)))) == -1
        if i:
            assert attrs(outs=tuple(None if j == i else t for j, t in enumerate((asum, tp, tf, tc)))) == -1
    assert attrs(a=None, Cn=0, outs=(None, tp, tf, tc)) == 0                            # C == 0: no table, no sums
    assert attrs(a=None, Cn=0, ins=(None,) * 4, Rr=0, outs=(None,) * 4) == 0
    vals, ps, pm = torch.zeros(R, 3, device=dev), torch.zeros(N_POINTS, 3, device=dev), torch.zeros(N_POINTS, device=dev)

    def lift(v=vals, Cn=3, f=None, ins=(bw, w, pidx, hit), Rr=R, SR=16, K=8, n=N_POINTS, s=ps, m=pm):
        return lib.pnerf_lift_to_points(P(v), Cn, P(f), *[P(t) for t in ins], Rr, SR, K, n, P(s), P(m), ops._stream())
    assert lift() == 0
    assert lift(Cn=9) == -4 and lift(Cn=-1) == -1
    assert lift(K=0) == -1 and lift(K=17) == -1 and lift(SR=0) == -1 and lift(Rr=-1) == -1 and lift(n=0) == -1
    assert lift(v=None) == -1 and lift(s=None) == -1 and lift(m=None) == -1
    for i in range(4):
        assert lift(ins=tuple(None if j == i else t for j, t in enumerate((bw, w, pidx, hit)))) == -1
    assert lift(v=None, Cn=0, s=None) == 0
    assert lift(v=None, Cn=0, ins=(None,) * 4, Rr=0, s=None, m=None) == 0
    with pytest.raises(ValueError, match="blend_w"):
        ops.ray_attributes(attr, bw[:, :8].contiguous(), w, pidx, hit)
    with pytest.raises(ValueError, match="sample_pidx"):
        ops.ray_attributes(attr, bw, w, pidx.float(), hit)
    with pytest.raises(ValueError, match="256"):
        ops.ray_attributes(torch.zeros(N_POINTS, 257, device=dev), bw, w, pidx, hit)
    with pytest.raises(ValueError, match="values"):
        ops.lift_to_points(torch.zeros(R, 9, device=dev), None, bw, w, pidx, hit, N_POINTS)
    with pytest.raises(ValueError, match="ray_factor"):
        ops.lift_to_points(None, torch.zeros(R + 1, device=dev), bw, w, pidx, hit, N_POINTS)


# ------------------------------------------------------------------------------------------------- 2. through the model
def model_tables(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g), torch.ones(n, 1)


def oracle_maps(weight, blend_w, pidx, attr):
    """the restatement on an oracle render's own tensors over its R'' hit rays, float64: dict(attr_sum, top_point, top_contrib, near)"""
    w, bw, p = weight.double().numpy(), blend_w.double().numpy(), pidx.numpy().astype(np.int64)
    Rh = w.shape[0]
    valid = p >= 0
    g = np.where(valid, bw[:, :, None] * w, 0.0).reshape(Rh, -1)
    pf = np.where(valid, p, 0).reshape(Rh, -1)
    s = (g[:, :, None] * attr.double().numpy()[pf]).sum(1)
    idx = g.argmax(1)
    rows = np.arange(Rh)
    mx = g[rows, idx]
    tp = np.where(mx > 0, pf[rows, idx], -1)
    other = np.where(pf != tp[:, None], g, 0.0).max(1)                        # the largest g of ANOTHER point
    near = (mx > 0) & (other >= mx * (1 - NEAR))
    return dict(attr_sum=s, top_point=tp, top_contrib=np.where(mx > 0, mx, 0.0), near=near)


def device_maps(model, d, attr):
    from pointnerf_amd import ops
    dn, dense, _ = C.dense_render(model, d)
    got = ops.ray_attributes(attr, dn["blend_w"], dn["weight"], dense["sample_pidx"], dense["ray_hit"])
    return got, dn, dense


def compare_maps(got, hit, ref, tag, near_share=0.02):
    n_hit = int(hit.sum())
    n_near = int(ref["near"].sum())
    assert n_near <= near_share * n_hit, (tag, n_near, n_hit)
    ok = ~ref["near"]
    e = dict(attr_sum=float(np.abs(got["attr_sum"].cpu().numpy()[hit].astype(np.float64) - ref["attr_sum"]).max()),
             top_contrib=float(np.abs(got["top_contrib"].cpu().numpy()[hit].astype(np.float64) - ref["top_contrib"])[ok].max()))
    print(tag, "errors %s; near %d of %d" % ({k: "%.2e" % v for k, v in e.items()}, n_near, n_hit))
    assert e["attr_sum"] <= BAR and e["top_contrib"] <= BAR, (tag, e)
    assert np.array_equal(got["top_point"].cpu().numpy()[hit][ok], ref["top_point"][ok]), tag
    return e


def check_own_tensors(got, dn, dense, n_points):
    """top_* bit for bit numpy on the device's own dense tensors"""
    bw, w = dn["blend_w"].cpu().numpy(), dn["weight"].cpu().numpy()
    pidx, hit = dense["sample_pidx"].cpu().numpy(), dense["ray_hit"].cpu().numpy()
    Rr, SR, K = w.shape
    _, g32, _, _ = entries(bw.reshape(Rr, SR), w, pidx.reshape(Rr, SR, K), hit, n_points)
    tp, tf, tc = pick(g32, pidx.reshape(Rr, -1))
    assert np.array_equal(got["top_point"].cpu().numpy(), tp) and np.array_equal(got["top_flat"].cpu().numpy(), tf)
    assert np.array_equal(got["top_contrib"].cpu().numpy().view(np.int32), tc.view(np.int32))
    miss = hit <= 0
    assert (tp[miss] == -1).all() and float(got["attr_sum"].cpu()[torch.from_numpy(miss)].abs().sum()) == 0.0


def check_model(name, shift, dev):
    from pointnerf_amd import ops
    full = C.full_render(name, shift)
    n = full["case"][1].shape[0]
    rgb, ones = model_tables(n)
    pidx = full["q"]["sample_pidx"][0]
    ref = oracle_maps(full["weight"][0], full["blend_w"], pidx, rgb)
    model, d = C.build_model(full["case"], dev)
    got, dn, dense = device_maps(model, d, rgb.to(dev))
    hit = (dense["ray_hit"] > 0).cpu().numpy()
    assert torch.equal((dense["ray_hit"] > 0).cpu()[None].to(torch.int8), full["ray_mask"])
    compare_maps(got, hit, ref, "%s +%g:" % (name, shift))
    check_own_tensors(got, dn, dense, n)
    # the table of ones: the accumulated opacity of ops.ray_geometry on the same render
    one = ops.ray_attributes(ones.to(dev), dn["blend_w"], dn["weight"], dense["sample_pidx"], dense["ray_hit"])
    opt, inp = full["case"][0], full["case"][3]
    cam = ops.make_camera(inp["campos"][0].numpy(), inp["camrotc2w"][0].numpy(), opt.vsize[2], opt.raydist_mode_unit)
    acc = ops.ray_geometry(cam, dense["sample_loc"], dense["sample_nn"], dense["ray_hit"], dn["opacity"], dn["blend_w"])["acc"].cpu().numpy().astype(np.float64)
    SR, K = int(opt.SR), int(opt.K)
    diff = np.abs(one["attr_sum"][:, 0].cpu().numpy().astype(np.float64) - acc)
    print("%s +%g: ones table against acc: %.3g of a bound of %.3g" % (name, shift, (diff / np.maximum(acc, 1e-300)).max(), (SR * K + K + 2) * U))
    assert (diff <= (SR * K + K + 2) * U * acc).all()
    assert torch.equal(one["top_point"], got["top_point"]) and torch.equal(one["top_contrib"], got["top_contrib"])


def check_cut_route(dev):
    """small_k8 +600, c = 0.1, stage 2: unshaded samples carry blend_w = weight = 0, so nothing is special-cased"""
    name, shift, c, B = "small_k8", 600.0, 0.1, 2
    full = C.full_render(name, shift)
    n = full["case"][1].shape[0]
    rgb, _ = model_tables(n)
    model, d = C.build_model(full["case"], dev)
    uncut, _, dense = device_maps(model, d, rgb.to(dev))
    model.transmittance_cutoff, model.cutoff_stage = c, B
    got, dn, dense = device_maps(model, d, rgb.to(dev))
    assert model.last_stats["rays_cut"] > 50
    change = float((got["attr_sum"] - uncut["attr_sum"]).abs().max())
    print("cut route c=%g B=%d: attr_sum change vs uncut %.3g (bound %.3g)" % (c, B, change, c * float(rgb.abs().max())))
    assert 0 < change < c * float(rgb.abs().max())
    cut = C.cut_of(full, c, B)
    ref = oracle_maps(cut["weight"], cut["blend_w"], full["q"]["sample_pidx"][0], rgb)
    hit = (dense["ray_hit"] > 0).cpu().numpy()
    near = cut["near"].numpy()
    assert int(near.sum()) <= 0.02 * near.size
    err = np.abs(got["attr_sum"].cpu().numpy()[hit].astype(np.float64) - ref["attr_sum"])[~near].max()
    print("cut route: attr_sum against the cut restatement %.2e, near %d" % (err, int(near.sum())))
    assert err <= BAR
    check_own_tensors(got, dn, dense, n)


def check_frames(dev, name="small_k8"):
    case, frames, r = E.reference(name)
    n = case[1].shape[0]
    rgb, _ = model_tables(n)
    ref = oracle_maps(r["weight"][0], r["blend_weight"][0, ..., 0], r["query"]["sample_pidx"][0], rgb)
    model, d = E.build_model(name, dev, frames)
    got, dn, dense = device_maps(model, d, rgb.to(dev))
    compare_maps(got, (dense["ray_hit"] > 0).cpu().numpy(), ref, "frames %s:" % name)


# ------------------------------------------------------------------------------------------------- 3. the module
def image_model(dev):
    """the 24 x 24 block of cutoff_case.IMAGE (x0 = 404: some rays miss) -> (model, d, intrinsic, h, w, state dict of the cloud)"""
    from pointnerf_amd import scenes
    from oracle import pyref
    I = C.IMAGE
    opt, xyz, attrs, _, mlp = C.shifted_case(I["name"], I["shift"])
    inp = dict(pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=I["x0"], y0=I["y0"], size=I["size"])))
    intr = inp["intrinsic"][0].clone()
    intr[0, 2] -= float(I["x0"]); intr[1, 2] -= float(I["y0"])
    model, d = C.build_model((opt, xyz, attrs, inp, mlp), dev)
    state = {"neural_points.xyz": xyz, **{"neural_points." + k: v for k, v in attrs.items()}}
    return model, d, intr, I["size"], I["size"], state


def _chunk_tensors(model, d, intr, h, w, chunk):
    """the dense tensors of the chunks render_point_maps / lift_image walk, concatenated over the image's rays"""
    from pointnerf_amd import eval_loop
    pix = eval_loop.pixel_grid(h, w, d["campos"].device)
    parts = []
    for k in range(0, h * w, chunk):
        raydir = eval_loop.rays_from_pixels(pix[:, k:k + chunk], intr.to(pix.device), d["camrotc2w"])
        with torch.no_grad():
            t = model.render_dense(d["campos"], raydir, d["camrotc2w"], d["near"], d["far"], d["bg_color"], train=False)
        parts.append((t[3].clone(), t[5].clone(), t[7]["sample_pidx"].clone(), t[7]["ray_hit"].clone()))
    return [torch.cat([p[i] for p in parts]).contiguous() for i in range(4)]


def check_module(dev):
    from pointnerf_amd import editing, ops, point_maps
    model, d, intr, h, w, state = image_model(dev)
    chunk = C.IMAGE["chunk"]
    assert h * w > 2 * chunk
    n = state["neural_points.xyz"].shape[0]
    rgb, _ = model_tables(n)
    a = (d["campos"], d["camrotc2w"], intr, h, w, d["near"], d["far"])
    bw, wt, pidx, hit = _chunk_tensors(model, d, intr, h, w, chunk)
    want = ops.ray_attributes(rgb.to(dev), bw, wt, pidx, hit)
    hitb = hit > 0
    assert 50 < int(hitb.sum()) < h * w - 20                                   # rays that hit and rays that miss
    with torch.enable_grad():                                                  # the functions are no_grad whatever the caller's mode
        table = rgb.to(dev).requires_grad_(True)
        maps = point_maps.render_point_maps(model, table, *a, bg_color=d["bg_color"], chunk=chunk)
        values = want["attr_sum"].view(h, w, 3).clone().requires_grad_(True)
        mask = torch.zeros(h, w, dtype=torch.bool, device=dev)
        mask[:, : w // 2] = True
        psum, pmass = point_maps.lift_image(model, values, *a, mask=mask, chunk=chunk)
    for t in list(maps.values()) + [psum, pmass]:
        assert t.grad_fn is None and not t.requires_grad
    assert sorted(maps) == ["attr", "hit", "top_contrib", "top_point"]
    assert tuple(maps["attr"].shape) == (h, w, 3) and maps["top_point"].dtype == torch.int32 and maps["hit"].dtype == torch.bool
    assert torch.equal(maps["attr"].reshape(-1, 3), want["attr_sum"]) and torch.equal(maps["top_point"].reshape(-1), want["top_point"])
    assert torch.equal(maps["top_contrib"].reshape(-1), want["top_contrib"]) and torch.equal(maps["hit"].reshape(-1), hitb)
    miss = ~hitb
    assert float(maps["attr"].reshape(-1, 3)[miss].abs().sum()) == 0.0 and (maps["top_point"].reshape(-1)[miss] == -1).all()
    assert float(maps["top_contrib"].reshape(-1)[miss].abs().sum()) == 0.0
    pick_only = point_maps.render_point_maps(model, None, *a, chunk=chunk)
    assert sorted(pick_only) == ["hit", "top_contrib", "top_point"] and torch.equal(pick_only["top_point"], maps["top_point"])
    # lift_image against the float64 restatement on the same chunks' tensors, and against the one-call op within the same bound
    valid, g32, g64, p = entries(bw.cpu().numpy(), wt.cpu().numpy(), pidx.cpu().numpy(), hit.cpu().numpy(), n)
    v_np, m_np = values.detach().reshape(-1, 3).cpu().numpy(), mask.reshape(-1).float().cpu().numpy()
    mass, a_mass, sums, a_sums, n_p = lift_sums(valid, g64, p, m_np, v_np, n)
    one_s, one_m = ops.lift_to_points(values.detach().reshape(-1, 3).contiguous(), mask.reshape(-1).float(), bw, wt, pidx, hit, n)
    for gs, gm in ((psum, pmass), (one_s, one_m)):
        assert tuple(gs.shape) == (n, 3) and tuple(gm.shape) == (n,)
        em, es = np.abs(gm.cpu().numpy().astype(np.float64) - mass), np.abs(gs.cpu().numpy().astype(np.float64) - sums)
        assert (em <= (n_p + 3) * U * a_mass).all() and (es <= (n_p + 3)[:, None] * U * a_sums).all()
        assert (gm.cpu().numpy()[n_p == 0] == 0).all()
    assert 0 < int((n_p > 0).sum()) < n
    # a second view into the same accumulators adds up; view_contribution is the mass without values or mask
    both = point_maps.lift_image(model, values.detach(), *a, mask=mask, out=(psum.clone(), pmass.clone()), chunk=chunk)
    # |both - 2 mass| <= (2 n_p + 3) u 2 A and |pmass - mass| <= (n_p + 3) u A, so |both - 2 pmass| <= (6 n_p + 12) u A per point
    assert (np.abs(both[1].cpu().numpy().astype(np.float64) - 2 * pmass.cpu().numpy().astype(np.float64)) <= (6 * n_p + 12) * U * a_mass).all()
    view = dict(campos=d["campos"], camrotc2w=d["camrotc2w"], intrinsic=intr[None], near=d["near"], far=d["far"])
    vis = point_maps.view_contribution(model, [view, view], h, w, chunk=chunk)
    m1, a1, _, _, n1 = lift_sums(valid, g64, p, None, None, n)
    assert (np.abs(vis.cpu().numpy().astype(np.float64) - 2 * m1) <= (2 * n1 + 3) * U * 2 * a1).all()
    # the selection helpers: exactly what compose_parts(inds=...) takes
    sel = point_maps.points_from_pick(maps["top_point"], mask, n)
    tp = maps["top_point"].cpu().numpy()[mask.cpu().numpy()]
    want_sel = np.zeros(n, bool)
    want_sel[tp[tp >= 0]] = True
    assert sel.dtype == torch.bool and np.array_equal(sel.cpu().numpy(), want_sel) and 0 < int(sel.sum()) < n
    t = float(np.median(mass[n_p > 0]))
    by_mass = point_maps.points_from_mass(pmass, t)
    assert by_mass.dtype == torch.bool and 0 < int(by_mass.sum()) < int((n_p > 0).sum())
    for s in (sel, by_mass):
        part = editing.compose_parts([(state, s.cpu(), None)])
        assert part[0].shape[0] == int(s.sum()) and part[5].shape[0] == int(s.sum())
