"""GPU: the eight tmix_vpred_step* entries (csrc/video_step.hip: one element kernel) at ONE shape, each against its numpy restatement
by np.array_equal -- guidance.vpred_rescaled_step_reference / vpred_rescaled_multistep_reference, with three different factors for the _rs entries and
factors of 1.0 for their parents (tests/test_video_rescale_cpu.py ties those to the older restatements).

S, C, F, hw = 3, 4, 3, 29131: n = 1,048,716 > 4096 workgroups x 256 threads = 1,048,576, so the capped grid takes a second element in EVERY form; hw is odd
and F divides nothing, so a wrong plan-row offset, a wrong i / per or a conditional half read at the wrong base shows; the three videos carry the
factors 0.5, 1.0 and 1.75, so a factor taken from the wrong video shows.  The dense forms run in f32, f16 and bf16; the device forms on fp32 plan rows
with a padded clip stride (NaN in the padding) and the two CFG halves in separate buffers.  The multistep forms run a second-order step (c1 != 0) on a
random history and a first-order step on a history of NaN.  out and x0_prev sit in guard-band frames."""
import functools

import numpy as np
import pytest
import torch

from layout_frames import Frame, dense_guarded
from test_video_solver_gpu import DT, G, ORDERS, S1, SA

pytestmark = pytest.mark.gpu

NF = np.float32
F32 = torch.float32
S, C, F, HW = 3, 4, 3, 29131
PER = C * F * HW
N = S * PER
FACTORS = (0.5, 1.0, 1.75)
AN = NF(0.2871)
SAN, S1N = np.sqrt(AN), np.sqrt(NF(1) - AN)
ENTRIES = [(ms, rs, dev) for dev in (False, True) for ms in (False, True) for rs in (False, True)]


def _name(e):
    ms, rs, dev = e
    return "tmix_vpred_step" + ("_ms" if ms else "") + ("_rs" if rs else "") + ("_dev" if dev else "")


@functools.lru_cache(maxsize=None)
def _data(dt):
    """-> x [S, PER], v [2S, PER] (fp32 copies of values of the dtype), prev [S, PER] fp32: numpy, shared and never written"""
    rng = np.random.RandomState(2051)
    q = lambda a: torch.from_numpy(a.astype(NF)).to(DT[dt][0]).float().numpy()
    x, v, prev = q(rng.randn(S, PER)), q(rng.randn(2 * S, PER)), rng.randn(S, PER).astype(NF)
    for a in (x, v, prev):
        a.setflags(write=False)
    return x, v, prev


@functools.lru_cache(maxsize=None)
def _want(dt, kind, rs):
    """the restatement of one (dtype, kind, rescale) -> (out, x0) [S, PER]; the device forms share the f32 ones"""
    from tweediemix_amd import guidance as GD
    x, v, prev = _data(dt)
    fac = np.asarray(FACTORS if rs else (1.0,) * S, NF)
    if kind == "ddim":
        return GD.vpred_rescaled_step_reference(x, v, fac, G, SA, S1, SAN, S1N, DT[dt][1])
    hist = np.full_like(prev, np.nan) if kind == "first" else prev
    return GD.vpred_rescaled_multistep_reference(x, v, hist, fac, G, SA, S1, *ORDERS[kind], DT[dt][1])


def _p(t):
    return None if t is None else t.data_ptr()


def _rows(a):
    """pipeline layout [S, PER] = [S][C][F][hw] numpy -> plan prediction rows [S, F * C, hw] on the device"""
    return torch.tensor(a).cuda().reshape(S, C, F, HW).permute(0, 2, 1, 3).reshape(S, F * C, HW)


@pytest.mark.parametrize("entry", ENTRIES, ids=_name)
def test_entry_equals_its_restatement(entry):
    from tweediemix_amd import lib as L
    lib = L.load()
    ms, rs, dev = entry
    fn = getattr(lib, _name(entry))
    st = torch.cuda.current_stream().cuda_stream
    assert 4096 * 256 < N < 4096 * 256 + 256
    fac = Frame.of(torch.tensor([FACTORS], dtype=F32, device="cuda"), name="factors").seal()
    facs = (_p(fac.view),) if rs else ()
    for dt in (["f32"] if dev else list(DT)):
        tdt = DT[dt][0]
        x, v, prev = _data(dt)
        for kind in ((["second", "first"] if dt == "f32" else ["second"]) if ms else ["ddim"]):
            what = (_name(entry), dt, kind)
            hist = torch.full((S * C * F, HW), float("nan"), device="cuda") if kind == "first" else torch.tensor(prev).cuda().reshape(S * C * F, HW)
            hf = Frame.of(hist, name="x0_prev")
            hists = (_p(hf.view),) if ms else ()
            if not ms:
                hf.seal()
            out = dense_guarded((S * C * F, HW), tdt, rows=8, device="cuda", name="x" if dev else "out")
            if dev:                                                     # in place on the fp32 state; the halves in two buffers, clips 24 floats apart
                out.view.copy_(torch.tensor(x).reshape(S * C * F, HW))
                stride = PER + 24
                vu = Frame.of(_rows(v[:S]), batch_stride=stride, name="v_u").seal()
                vc = Frame.of(_rows(v[S:]), batch_stride=stride, name="v_c").seal()
                tail = ORDERS[kind] + (G, 0.0) if ms else (SAN, S1N, G, 0.0, 0.0)
                prm = Frame.of(torch.tensor([[501.0, SA, S1, *tail]], dtype=F32, device="cuda"), name="params").seal()
                inputs = (vu, vc, prm)
                rc = fn(_p(out.view), _p(vu.view), stride, _p(vc.view), stride, *hists, _p(prm.view), S, C, F, HW, *facs, st)
            else:
                xin = Frame.of(torch.tensor(x).to(tdt).cuda(), name="x").seal()
                vin = Frame.of(torch.tensor(v).to(tdt).cuda().reshape(1, -1), name="v").seal()
                inputs = (xin, vin)
                shape = (S, PER) if rs else (N,)
                tail = ORDERS[kind] if ms else (float(SAN), float(S1N))
                rc = fn(_p(xin.view), _p(vin.view), _p(out.view), *hists, getattr(L, dt.upper()), *shape, G, float(SA), float(S1), *tail, *facs, st)
            assert rc == 0, (what, lib.tmix_last_error_string())
            torch.cuda.synchronize()
            out.assert_untouched()
            out.assert_all_written()
            hf.assert_untouched() if ms else hf.assert_unchanged()
            for f in inputs + (fac,):
                f.assert_unchanged()
            want, want0 = _want(dt, kind, rs)
            got = out.view.float().cpu().numpy().reshape(S, PER)
            assert np.isfinite(got).all(), what
            assert np.array_equal(got, want), (what, int((got != want).sum()))
            if ms:
                got0 = hf.view.cpu().numpy().reshape(S, PER)
                assert np.array_equal(got0, want0), (what, int((got0 != want0).sum()))
