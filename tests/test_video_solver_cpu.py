"""CPU: few-step VIDEO sampling without a GPU -- VideoSchedule's 'logsnr' grid, next_alpha and the injection mapping, the video
table's coefficient helper and the numpy restatement of tmix_vpred_step_ms (tweediemix_amd/solver.py), the phase rule (video.SolverPhase), the
Gaussian toy on the stand-in table, the declarations and argument errors of the two entries (reported on the host before any launch) and the
command-line refusals.  Nothing here opens the GPU."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from video_solver_cases import NF, TOY_BOUND, TOY_CASES, TOY_PAYS, TOY_WORST, standin_schedule, standin_table, toy_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (2, 3, 10, 20, 50)


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n", NS + (7, 1000))
def test_leading_spacing_is_the_schedule_of_today(n):
    from tweediemix_amd import video as V
    acp, kw = standin_table()
    a, b = V.VideoSchedule(acp, n, **kw), V.VideoSchedule(acp, n, **kw, spacing="leading")
    assert a.spacing == b.spacing == "leading" and a.skip == b.skip == 1000 // n and a.n == b.n == n
    assert np.array_equal(a.timesteps, b.timesteps) and a.timesteps.dtype == np.int64
    assert np.array_equal(a.timesteps, (np.arange(n) * (1000 // n))[::-1] + 1)
    assert a.final_alpha_cumprod == b.final_alpha_cumprod == acp[0]
    for t in a.timesteps:
        if t < 1000:                                           # n = 1000 starts at t = 1000, outside the table, as it always did
            assert a.alpha(t) == b.alpha(t) == acp[t]
        assert a.next_alpha(t) == b.next_alpha(t) == a.alpha(int(t) - a.skip)
    assert a.next_alpha(1) == acp[0] and a.next_alpha(500) == a.alpha(500 - a.skip)      # off the grid too
    for ratio in (0, 0.02, 0.1, 0.5):
        assert a.injection_schedule(ratio) == b.injection_schedule(ratio) == set(int(t) for t in a.timesteps[:int(n * ratio)])


def _lam(sch, t):
    a = float(sch.acp[t])
    return 0.5 * math.log(a / (1.0 - a))


@pytest.mark.parametrize("n", NS)
def test_logsnr_grid_properties(n):
    s, lead = standin_schedule(n, "logsnr"), standin_schedule(n)
    ts, t_hi = [int(t) for t in s.timesteps], int(lead.timesteps[0])
    assert len(ts) == n and s.timesteps.dtype == np.int64
    assert ts[0] == t_hi and ts[-1] == 1 and all(a > b for a, b in zip(ts, ts[1:]))
    assert s.skip is None and s.spacing == "logsnr" and s.n == n
    assert np.array_equal(s.acp, lead.acp) and s.final_alpha_cumprod == lead.final_alpha_cumprod
    for i, t in enumerate(ts):
        assert s.alpha(t) == s.acp[t]                            # the UN-shifted table
        assert s.next_alpha(t) == (s.acp[ts[i + 1]] if i + 1 < n else s.final_alpha_cumprod)
    with pytest.raises(ValueError):
        s.next_alpha(t_hi + 1)                                   # this spacing has no stride to fall back on
    lam = [_lam(s, t) for t in ts]
    assert all(b > a for a, b in zip(lam, lam[1:]))
    # nearest in lambda before the two monotonic passes (ties: the smaller t)
    target = [lam[0] + i * (_lam(s, 1) - lam[0]) / (n - 1) for i in range(n)]
    all_lam = [_lam(s, t) for t in range(1, t_hi + 1)]
    nearest = []
    for tg in target:
        d = [abs(v - tg) for v in all_lam]
        nearest.append(1 + d.index(min(d)))
    if all(a > b for a, b in zip(nearest, nearest[1:])):         # no collision: the grid IS the nearest integers
        assert ts == nearest
    else:                                                        # n = 50 collides near t = 1: the two passes, restated
        fixed = [t_hi] + nearest[1:]
        for i in range(1, n):
            fixed[i] = min(fixed[i], fixed[i - 1] - 1)
        fixed[-1] = 1
        for i in range(n - 2, -1, -1):
            fixed[i] = max(fixed[i], fixed[i + 1] + 1)
        assert n == 50 and ts == fixed
    if n <= 20:
        assert ts == nearest
        for i, t in enumerate(ts[1:-1], 1):                      # uniform to within the integer grid: half the local lambda spacing
            half = 0.5 * max(_lam(s, t - 1) - _lam(s, t), _lam(s, t) - _lam(s, t + 1))
            assert abs(lam[i] - target[i]) <= half * (1 + 1e-12), (n, i, t)


def test_logsnr_grid_pinned_and_errors():
    from tweediemix_amd import video as V
    acp, kw = standin_table()
    assert [int(t) for t in standin_schedule(10, "logsnr").timesteps] == [901, 801, 625, 397, 210, 100, 45, 18, 6, 1]
    assert [int(t) for t in standin_schedule(15, "logsnr").timesteps] == [925, 879, 808, 701, 560, 405, 269, 169, 102, 60, 34, 18, 9, 4, 1]
    assert [int(t) for t in standin_schedule(2, "logsnr").timesteps] == [501, 1]
    with pytest.raises(ValueError, match="logsnr"):
        V.VideoSchedule(acp, 1, **kw, spacing="logsnr")         # one timestep has no interval
    with pytest.raises(ValueError, match="logsnr"):
        V.VideoSchedule(acp, 1000, **kw, spacing="logsnr")      # t_hi = 1000 lies outside the table
    with pytest.raises(ValueError, match="logsnr"):
        V.VideoSchedule(acp[:8], 8, steps_offset=1, spacing="logsnr")      # skip = 1: t_hi = 8, outside an 8-entry table
    with pytest.raises(ValueError, match="logsnr"):
        V.VideoSchedule(acp[:9], 9, steps_offset=0, spacing="logsnr")      # n = 9 > t_hi = 8
    assert [int(t) for t in V.VideoSchedule(acp[:9], 8, steps_offset=1, spacing="logsnr").timesteps] == [8, 7, 6, 5, 4, 3, 2, 1]     # n == t_hi fits
    assert list(V.VideoSchedule(acp, 1, **kw).timesteps) == [1]            # 'leading' takes what it always took
    with pytest.raises(ValueError, match="spacing"):
        V.VideoSchedule(acp, 10, **kw, spacing="trailing")
    one = V.VideoSchedule(acp, 10, steps_offset=1, set_alpha_to_one=True, spacing="logsnr")
    assert one.next_alpha(1) == 1.0 and one.final_alpha_cumprod == 1.0


@pytest.mark.parametrize("n", [10, 20, 50])
def test_injection_mapping_keeps_the_noise_range(n):
    lead, s = standin_schedule(n), standin_schedule(n, "logsnr")
    ts = [int(t) for t in s.timesteps]
    for ratio in (0, 0.02, 0.1, 0.5):
        k = int(n * ratio)
        got = s.injection_schedule(ratio)
        if k == 0:
            assert got == set()
            continue
        floor = int(lead.timesteps[k - 1])
        assert got == {t for t in ts if t >= floor} and ts[0] in got
        assert got == set(ts[:len(got)])                         # a prefix of the grid
        if k == 1:
            assert got == {ts[0]}                                # the first step, as today
    from tweediemix_amd import video as V
    assert V.injection_active(1000, set()) and not V.injection_active(999, set()) and not V.injection_active(1000, None)
    if n == 10:
        assert s.injection_schedule(0.5) == {901, 801, 625}      # leading: 901 .. 501


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("spacing,n", [("logsnr", 10), ("logsnr", 50), ("leading", 10), ("leading", 50)])
def test_first_order_coefficients_are_the_ddim_move(spacing, n):
    """cx x + c0 x0 with x0 = sa x - s1 v equals sa' x0 + s1' (sa v + s1 x) in fp64, to 1e-12 relative, for any x and v"""
    from tweediemix_amd import solver as SV
    s = standin_schedule(n, spacing)
    rng = np.random.RandomState(n)
    for t in s.timesteps:
        a, an = s.alpha(int(t)), s.next_alpha(int(t))
        cx, c0, c1 = SV.multistep_coeffs64(None, a, an, False)
        assert c1 == 0.0
        assert SV.video_multistep_coeffs(int(t), None, a, an, False) == tuple(float(NF(v)) for v in (cx, c0, c1))
        sa, s1, san, s1n = math.sqrt(float(a)), math.sqrt(1 - float(a)), math.sqrt(float(an)), math.sqrt(1 - float(an))
        for x, v in rng.randn(8, 2):
            x0, eps = sa * x - s1 * v, sa * v + s1 * x
            want = san * x0 + s1n * eps
            scale = abs(san * x0) + abs(s1n * eps) + abs(cx * x) + abs(c0 * x0)
            assert abs(cx * x + c0 * x0 - want) <= 1e-12 * scale, (int(t), a, an)


def test_coefficient_helper_edge_cases():
    from tweediemix_amd import solver as SV, video as V
    acp, kw = standin_table()
    assert acp[999] == 0.0
    assert SV.video_multistep_coeffs(1, 0.9, 0.99, 1.0, True) == (0.0, 1.0, 0.0)          # a_next == 1: x0, what DDIM gives there; first order
    assert SV.video_multistep_coeffs(1, None, 0.99, np.float32(1.0), False) == (0.0, 1.0, 0.0)
    assert SV.video_multistep_coeffs(21, 0.5, 0.6, 0.7, True) == SV.multistep_coeffs(0.5, 0.6, 0.7, True)
    with pytest.raises(ValueError, match=r"alpha\(999\)"):
        SV.video_multistep_coeffs(999, None, acp[999], acp[979], False)
    # through the phase bookkeeping: the zero-SNR table's t = 999 and a timestep outside the table
    ph = V.SolverPhase(V.VideoSchedule(acp, 50, **kw))
    with pytest.raises(ValueError, match=r"alpha\(999\)"):
        ph.coeffs(999)
    with pytest.raises(ValueError, match=r"alpha\(1000\)"):
        ph.coeffs(1000)
    with pytest.raises(ValueError, match=r"alpha\(1000\)"):                                 # n = 1000 on 'leading' starts at t = 1000
        V.SolverPhase(V.VideoSchedule(acp, 1000, **kw)).coeffs(1000)
    one = V.VideoSchedule(acp, 10, steps_offset=1, set_alpha_to_one=True, spacing="logsnr")
    ph = V.SolverPhase(one)
    cf = [ph.coeffs(int(t)) for t in one.timesteps]
    assert cf[-1] == (0.0, 1.0, 0.0) and all(c[2] < 0 for c in cf[1:-1]) and cf[0][2] == 0.0


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("lowp", [None, np.float16, "bf16"])
def test_restatement_x0_is_the_ddim_formulas_x0(lowp):
    """the x0 of solver.vpred_multistep_reference equals the x0 of the DDIM formula (oracle.tweedie_oracle.video_vpred_step's operations) by equality;
    the move is every product and sum on its own"""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import solver as SV
    rng = np.random.RandomState(3)
    lp = lowp if lowp is np.float16 else None
    q = (lambda a: a.astype(np.float16).astype(NF)) if lp else (lambda a: a)
    x, v, prev = q(rng.randn(2, 4, 3, 5, 7).astype(NF)), q(rng.randn(4, 4, 3, 5, 7).astype(NF)), rng.randn(2, 4, 3, 5, 7).astype(NF)
    at, g = NF(0.2345), 9.0
    sa, s1 = np.sqrt(at), np.sqrt(NF(1) - at)
    h = lambda a: TO._h(a, lp)
    vv = h(v[:2] + h(NF(g) * h(v[2:] - v[:2])))
    want0 = h(h(sa * x) - h(s1 * vv))
    # ... which is the x0 inside the oracle's DDIM step: with a_next = 1 that step returns sqrt(1) x0 + 0 eps
    assert np.array_equal(TO.video_vpred_step(x, v, g, at, NF(1.0), lp), h(h(NF(1) * want0) + h(NF(0) * h(h(sa * vv) + h(s1 * x)))))
    out, x0 = SV.vpred_multistep_reference(x, v, prev, g, sa, s1, 0.5, 0.25, -0.125, lowp)
    assert x0.dtype == NF and out.dtype == NF and np.array_equal(x0, want0)
    want = h(h(NF(0.5) * x) + h(h(NF(0.25) * want0) + h(NF(-0.125) * prev)))
    if lowp == "bf16":
        assert not np.array_equal(out, want)
        want = torch.from_numpy(want).bfloat16().float().numpy()                          # one rounding, at the store
    assert np.array_equal(out, want)
    out, x0 = SV.vpred_multistep_reference(x, v, np.full_like(prev, np.nan), g, sa, s1, 0.5, 0.25, 0.0, lowp)
    want = h(h(NF(0.5) * x) + h(NF(0.25) * want0))
    assert np.array_equal(out, torch.from_numpy(want).bfloat16().float().numpy() if lowp == "bf16" else want)      # c1 = 0: the history is not read
    assert np.array_equal(x0, want0)
    # a_next == 1: (0, 1, 0) gives x0 itself
    out, _ = SV.vpred_multistep_reference(x, v, prev, g, sa, s1, 0.0, 1.0, 0.0, lp)
    assert np.array_equal(out, want0 + NF(0))


# ------------------------------------------------------------------------------------------------ the Gaussian toy
@pytest.fixture(scope="module")
def toy_table():
    """{(m, c): {"ddim50": err, 10: err, 15: err, 20: err, "first10": err, "first20": err}}, computed once"""
    xT = np.random.RandomState(0).randn(4096)
    out = {}
    for m, c in TOY_CASES:
        row = {"ddim50": toy_run(m, c, 50, "leading", "ddim", xT)}
        for n in (10, 15, 20):
            row[n] = toy_run(m, c, n, "logsnr", "dpmpp2m", xT)
        for n in (10, 20):
            row[f"first{n}"] = toy_run(m, c, n, "logsnr", "dpmpp2m", xT, first_order_only=True)
        out[(m, c)] = row
        print(f"m = {m} c = {c}: DDIM leading n=50 {row['ddim50']:.3e}  2M logsnr n=10 {row[10]:.3e} ({row[10] / row['ddim50']:.3f})  "
              f"n=15 {row[15]:.3e} ({row[15] / row['ddim50']:.3f})  n=20 {row[20]:.3e} ({row[20] / row['ddim50']:.3f})  "
              f"first order n=10 {row['first10']:.3e} n=20 {row['first20']:.3e}")
    return out


@pytest.mark.parametrize("n", [10, 15, 20])
def test_gaussian_toy_2m_logsnr_against_ddim_leading_50(toy_table, n):
    """the error of 2M on the log-SNR grid at n over the error of DDIM 'leading' at n = 50, nine (m, c) cases, 4096 draws of x_T, with the sampler's
    fp32-rounded coefficients.  Re-measured (this draw), m = 0 / 0.7 / 3 by c = 0.2, 0.5, 1:
      n = 10: 0.377 0.808 0.906 / 0.393 0.855 0.950 / 0.433 0.961 1.133      n = 15: 0.212 0.440 0.524 / 0.218 0.457 0.541 / 0.231 0.491 0.605
      n = 20: 0.138 0.285 0.356 / 0.140 0.290 0.362 / 0.144 0.299 0.381
    The bound per n is the worst ratio times 1.25.  At n = 20 (0.476) and n = 15 (0.756) it is below 1: twenty, resp. fifteen calls cost less error than DDIM's
    fifty in every case.  At n = 10 the worst ratio is 1.133: FINDING -- on this table 2M at n = 10 does not beat DDIM at n = 50 in every case (it does in
    eight of nine); the n = 10 bound (1.416) only pins the measurement."""
    ratios = {k: row[n] / row["ddim50"] for k, row in toy_table.items()}
    for k, r in ratios.items():
        assert r < TOY_BOUND[n], (n, k, r)
    assert abs(max(ratios.values()) - TOY_WORST[n]) < 0.02, "the re-measured worst ratio left the value the bound was derived from"
    assert (TOY_BOUND[n] < 1.0) == (n in TOY_PAYS)
    if n in TOY_PAYS:
        assert all(r < 1.0 for r in ratios.values())


def test_gaussian_toy_second_order_is_what_helps(toy_table):
    """the same grid with first-order steps only (c1 = 0 throughout) is worse in every case, at n = 10 and at n = 20"""
    for k, row in toy_table.items():
        assert row[10] < row["first10"] and row[20] < row["first20"], (k, row)


# ------------------------------------------------------------------------------------------------ phase rule
@pytest.mark.parametrize("spacing", ["logsnr", "leading"])
def test_phase_rule(spacing):
    """from the host's bookkeeping alone: second order exactly when the previous call was for the preceding schedule entry"""
    from tweediemix_amd import solver as SV, video as V
    s = standin_schedule(10, spacing)
    ts = [int(t) for t in s.timesteps]
    ph = V.SolverPhase(s)
    for i, t in enumerate(ts):
        cf = ph.coeffs(t)
        want = SV.multistep_coeffs(s.alpha(ts[i - 1]) if i else None, s.alpha(t), s.next_alpha(t), i > 0)
        assert cf == want and (cf[2] == 0.0) == (i == 0) and all(float(NF(v)) == v for v in cf), (i, t)
    # out of order
    ph = V.SolverPhase(s)
    order = [ph.coeffs(t)[2] == 0.0 for t in (ts[4], ts[5], ts[5], ts[3], ts[4], ts[6], ts[7])]
    assert order == [True, False, True, True, False, True, False]
    # a new trajectory starts first order; a refused step leaves no history
    assert ph.coeffs(ts[0])[2] == 0.0 and ph.coeffs(ts[1])[2] < 0
    with pytest.raises(ValueError):
        ph.coeffs(999)
    assert ph.coeffs(ts[2])[2] == 0.0
    if spacing == "leading":                                     # off the grid: first order, and the step behind it too
        assert ph.coeffs(ts[3])[2] < 0 and ph.coeffs(ts[4] + 7)[2] == 0.0 and ph.coeffs(ts[5])[2] == 0.0
    else:
        with pytest.raises(ValueError):
            ph.coeffs(ts[4] + 7)
    # the injection state does not enter: the rule has no such input
    assert set(vars(ph)) == {"schedule", "prev"}
    # the public hook for a caller that puts state and history in place itself
    ph.set_previous(ts[4])
    assert ph.coeffs(ts[5])[2] < 0
    ph.set_previous(ts[4])
    assert ph.coeffs(ts[6])[2] == 0.0
    ph.set_previous(None)
    assert ph.coeffs(ts[7])[2] == 0.0
    assert [s.index(t) for t in ts] == list(range(10)) and s.index(ts[0] + 1) is None


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_sample_loop_runs_without_autograd(solver, monkeypatch):
    """sample_loop calls the network under torch.no_grad(), as it always did, whatever the solver (the step kernels are replaced by recorders:
    no device)"""
    from tweediemix_amd import ops, video as V
    assert torch.is_grad_enabled()
    seen, steps = [], []
    monkeypatch.setattr(ops, "vpred_step", lambda x, v, *a, **k: (steps.append("ddim"), x)[1])
    monkeypatch.setattr(ops, "vpred_step_ms", lambda x, v, *a, **k: (steps.append("ms"), x)[1])
    w = torch.ones(1, requires_grad=True)

    def unet(xin, t):
        seen.append(torch.is_grad_enabled())
        out = xin * w
        assert not out.requires_grad
        return out
    V.sample_loop(unet, torch.zeros(1, 4, 2, 2, 2), standin_schedule(10, "logsnr"), 9.0, solver=solver)
    assert seen == [False] * 10 and steps == [{"ddim": "ddim", "dpmpp2m": "ms"}[solver]] * 10
    assert torch.is_grad_enabled()


def test_solver_argument_is_checked():
    from tweediemix_amd import video as V
    with pytest.raises(ValueError, match="solver='euler'"):
        V.sample_loop(None, torch.zeros(1, 4, 2, 2, 2), standin_schedule(10), 9.0, solver="euler")
    with pytest.raises(ValueError, match="solver='euler'"):
        V.VideoSampler(None, standin_schedule(10), 9.0, solver="euler")
    assert V.SOLVERS == ("ddim", "dpmpp2m") and V.SPACINGS == ("leading", "logsnr")


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
          "float": C.c_float}


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_entry_prototypes_match_their_ctypes_declarations():
    from tweediemix_amd import lib
    ddim, ms = _prototype("tmix_vpred_step"), _prototype("tmix_vpred_step_ms")
    assert [n for _t, n in ms] == ["x", "v", "out", "x0_prev", "dtype", "n", "g", "sa", "s1", "cx", "c0", "c1", "stream"]
    assert ms[:3] == ddim[:3] and ms[3] == ["float*", "x0_prev"] and ms[4:9] == ddim[3:8]
    dev, msd = _prototype("tmix_vpred_step_dev"), _prototype("tmix_vpred_step_ms_dev")
    assert msd == dev[:5] + [["float*", "x0_prev"]] + dev[5:]     # the DDIM entry's arguments with the history buffer behind the halves
    for name, proto in (("tmix_vpred_step_ms", ms), ("tmix_vpred_step_ms_dev", msd)):
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int and args == [_CTYPE[t] for t, _n in proto], name
        assert getattr(lib.load(), name).argtypes == args


def test_entries_validate_before_any_launch():
    from tweediemix_amd import lib
    l = lib.load()
    err = l.tmix_last_error_string
    f = 0x1000                                                  # never dereferenced: validation fails first
    ok = dict(x=f, v=f, out=f, prev=f, dt=lib.F32, n=64)

    def rc(**kw):
        a = dict(ok, **kw)
        return l.tmix_vpred_step_ms(a["x"], a["v"], a["out"], a["prev"], a["dt"], a["n"], 9.0, 0.6, 0.8, 0.9, 0.2, -0.1, None)
    assert rc(prev=None) == lib.EINVAL and b"x0_prev" in err()
    for k in ("x", "v", "out"):
        assert rc(**{k: None}) == lib.EINVAL and b"null" in err(), k
    assert rc(dt=7) == lib.EINVAL and b"dtype" in err() and rc(dt=-1) == lib.EINVAL
    assert rc(n=0) == lib.ESHAPE and rc(n=-5) == lib.ESHAPE
    okd = dict(x=f, vu=f, su=4 * 2 * 64, vc=f, sc=4 * 2 * 64, prev=f, prm=f, S=2, C=4, F=2, hw=64)

    def rcd(**kw):
        a = dict(okd, **kw)
        return l.tmix_vpred_step_ms_dev(a["x"], a["vu"], a["su"], a["vc"], a["sc"], a["prev"], a["prm"], a["S"], a["C"], a["F"], a["hw"], None)
    assert rcd(prev=None) == lib.EINVAL and b"x0_prev" in err()
    for k in ("x", "vu", "vc", "prm"):
        assert rcd(**{k: None}) == lib.EINVAL and b"null" in err(), k
    for bad in (dict(S=0), dict(C=0), dict(F=0), dict(hw=0)):
        assert rcd(**bad) == lib.ESHAPE, bad
    assert rcd(su=511) == lib.ESHAPE and b"clip stride" in err()
    assert rcd(sc=511) == lib.ESHAPE and rcd(su=0) == lib.ESHAPE


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    z = torch.zeros(1, 4, 2, 4, 4)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_ms(z, torch.zeros(2, 4, 2, 4, 4), 9.0, 0.5, (0.9, 0.2, 0.0), z.clone())
    with pytest.raises(lib.TmixError):
        ops.vpred_step_ms_dev(z, torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), z.clone(), torch.zeros(8))
    p = ops.video_step_params_ms(21, 9.0, np.float32(0.36), (0.9, 0.2, -0.1))
    assert p.dtype == torch.float32 and p.tolist() == [21.0, float(np.sqrt(NF(0.36))), float(np.sqrt(NF(1) - NF(0.36))), float(NF(0.9)), float(NF(0.2)),
                                                        float(NF(-0.1)), 9.0, 0.0]


# ------------------------------------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def rv():
    spec = importlib.util.spec_from_file_location("rv_solver_cpu", os.path.join(ROOT, "run_video.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_flags_and_refusals_come_before_the_gpu(rv, monkeypatch):
    opt = rv.build_parser().parse_args([])
    assert opt.solver == "ddim" and opt.timestep_spacing == "leading"
    sch = rv.checked_schedule(opt)
    assert sch.spacing == "leading" and sch.skip == 20 and int(sch.timesteps[0]) == 981
    opt = rv.build_parser().parse_args(["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_inference_steps", "10", "--synthetic"])
    assert (opt.solver, opt.timestep_spacing) == ("dpmpp2m", "logsnr")
    assert [int(t) for t in rv.checked_schedule(opt).timesteps][:3] == [901, 801, 625]
    for bad in (["--solver", "euler"], ["--timestep_spacing", "trailing"]):
        with pytest.raises(SystemExit):
            rv.build_parser().parse_args(bad)

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream", "current_device"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    base = ["--synthetic", "--tiny", "--height", "128", "--width", "64"]
    with pytest.raises(SystemExit, match=r"--timestep_spacing logsnr with --num_inference_steps 1\b"):
        rv.main(base + ["--timestep_spacing", "logsnr", "--num_inference_steps", "1"])
    with pytest.raises(SystemExit, match=r"--timestep_spacing logsnr with --num_inference_steps 1000\b"):
        rv.main(base + ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_inference_steps", "1000"])
    with pytest.raises(SystemExit, match=r"--solver dpmpp2m --timestep_spacing leading with --num_inference_steps 1000: .*alpha\(1000\)"):
        rv.main(base + ["--solver", "dpmpp2m", "--num_inference_steps", "1000"])
    with pytest.raises(SystemExit, match=r"--num_inference_steps 1000\b"):          # ... and before any rank is started
        rv.main(base + ["--solver", "dpmpp2m", "--num_inference_steps", "1000", "--gpus", "2", "--num_seeds", "2"])
