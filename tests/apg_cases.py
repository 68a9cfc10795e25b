"""Shared by tests/test_apg_cpu.py and tests/test_apg_gpu.py (adaptive projected guidance): the cases of the coefficient launches
with their bound, the kernel's partition order restated in numpy, and the inputs of one launch of tmix_fused_tweedie_step_apg_dev with their
restatement.  Nothing here touches the GPU at import."""
import numpy as np

from guidance_interval_cases import SEEDS64, mode_id, torch_dtype

NF = np.float32
MODES = ("fusion", "plain", "resample")
DTS = ("f32", "f16", "bf16")
RS_P, RS_THREADS = 32, 256                     # csrc/cfg_rescale.hip: one pass of the partials grid covers RS_P * RS_THREADS = 8192 elements
# n = 4 hw.  hw = 256: n = 1024, four of the 32 workgroups get elements, 28 none; hw = 2053: n = 8212, one pass plus a ragged tail of 20 elements;
# hw = 4100: n = 16400, two passes and a tail
SHAPES = ((16, 16), (1, 2053), (50, 82))
GS = (1.0, 7.5, 9.0, 30.0)
ETAS = (0.0, 0.3, 1.0)
NORMS = (0.0, 2.5, 15.0, 1e4)                  # no clip; a clip that binds on every shape; one that binds on the larger ones; one that never binds
ALPHAS = (0.2345, 0.9, 0.02)                   # alpha_bar of the step: sa = sqrt(a), s1 = sqrt(1 - a)


def _p(t):
    return None if t is None else t.data_ptr()


def used_rows(mode, K):
    return 1 if mode == "plain" else K


def sa_s1(a):
    a = NF(a)
    return float(np.sqrt(a)), float(np.sqrt(NF(1) - a))


def coeff_cases(mode, dt):
    """the launches of one (mode, eps dtype): shape x K in {1, 3} x rows in {used + 1, used + 2} x seeds in {1, 3}, cycling g x eta x R x alpha"""
    i = 7 * MODES.index(mode) + 23 * DTS.index(dt)
    out = []
    for h, w in SHAPES:
        for K in (1, 3):
            for spare in (0, 1):
                for seeds in (1, 3):
                    out.append(dict(mode=mode, dt=dt, h=h, w=w, K=K, rows=used_rows(mode, K) + 1 + spare, seeds=seeds, g=GS[i % 4], eta=ETAS[(i // 4) % 3],
                                    R=NORMS[(i // 12) % 4], alpha=ALPHAS[(i // 3) % 3], slot=6 + (i & 1), seed=2000 + i))
                    i += 5
    return out


def coeff_inputs(c):
    """(x [seeds, 4, h, w] fp32, eps tensor [seeds * rows, 4, h, w] of the eps dtype, its fp32 numpy copy, params list of 8 floats)"""
    import torch
    rng = np.random.RandomState(c["seed"])
    S, rows, h, w = c["seeds"], c["rows"], c["h"], c["w"]
    x = rng.randn(S, 4, h, w).astype(NF)
    eu = rng.randn(S, 1, 4, h, w)
    ec = eu + 0.5 * rng.randn(S, rows - 1, 4, h, w)
    eps_t = torch.from_numpy(np.concatenate([eu, ec], axis=1).reshape(S * rows, 4, h, w).astype(NF)).to(torch_dtype(c["dt"]))
    sa, s1 = sa_s1(c["alpha"])
    prm = [0.0] * 8
    prm[1], prm[2], prm[c["slot"]] = sa, s1, c["g"]
    return x, eps_t, eps_t.float().numpy(), [float(NF(v)) for v in prm]


def lowp_of(dt):
    return np.float16 if dt == "f16" else None


def coeffs_reference(c, x, eps, prm):
    """([seeds, rows-1, 2] fp32, [seeds, rows-1] fp64 bound on |A - A_ref|) from guidance.apg_coeffs_reference and the restatement's own sums:
    ulp32(A_ref) + 4 (g-1)(1-eta) n 2^-53 s sqrt(Sdd / Scc) -- the two sides form identical fp32 terms and differ in the order of n fp64 additions."""
    from tweediemix_amd import guidance as G
    S, rows = c["seeds"], c["rows"]
    n = x[0].size
    used = used_rows(c["mode"], c["K"])
    ref, bound = np.empty((S, rows - 1, 2), NF), np.zeros((S, rows - 1))
    g32, eta32 = float(NF(c["g"])), float(NF(c["eta"]))
    for sd in range(S):
        e = eps[sd * rows:(sd + 1) * rows]
        ref[sd] = G.apg_coeffs_reference(mode_id(c["mode"]), x[sd:sd + 1], e, c["K"], c["g"], prm[1], prm[2], c["eta"], c["R"], lowp_of(c["dt"]))
        sums = G.apg_sums_reference(x[sd:sd + 1], e, NF(prm[1]), NF(prm[2]), lowp_of(c["dt"]))
        for r in range(rows - 1):
            bound[sd, r] = float(np.spacing(np.abs(ref[sd, r, 0])))
            if r < used and np.isfinite(sums[r]).all() and sums[r, 2] > 0:
                _A, _B, s = G.apg_finalise(sums[r], c["g"], c["eta"], c["R"])
                bound[sd, r] += 4.0 * abs(g32 - 1.0) * (1.0 - eta32) * n * 2.0 ** -53 * s * np.sqrt(sums[r, 0] / sums[r, 2])
    return ref, bound


def partition_sums(tc, d):
    """(Sdd, Sdc, Scc) of ONE row in the order of apg_partials_kernel / apg_finalise_kernel: thread (p, tid) adds its elements p * 256 + tid +
    k * 8192 in k order; the wave64 butterfly (xor 32, 16, .., 1); the four waves in order; the 32 partials in index order.  Zeros pad the last
    pass: adding +0.0 changes no fp64 sum."""
    c64, d64 = np.asarray(tc, NF).astype(np.float64).reshape(-1), np.asarray(d, NF).astype(np.float64).reshape(-1)
    n = c64.size
    per = RS_P * RS_THREADS
    passes = (n + per - 1) // per
    out = []
    for prod in (d64 * d64, d64 * c64, c64 * c64):
        v = np.zeros(passes * per)
        v[:n] = prod
        v = v.reshape(passes, RS_P, RS_THREADS // 64, 64)
        acc = np.zeros(v.shape[1:])
        for k in range(passes):
            acc = acc + v[k]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., lane ^ m]
        part = acc[:, 0, 0]
        for wv in range(1, RS_THREADS // 64):
            part = part + acc[:, wv, 0]
        s = 0.0
        for p in range(RS_P):
            s = s + part[p]
        out.append(float(s))
    return out


def partition_coeffs(c, x, eps, prm):
    """[seeds, rows-1, 2] fp32: what the kernels compute, sum order included, restated in numpy"""
    from tweediemix_amd import guidance as G
    S, rows = c["seeds"], c["rows"]
    used = used_rows(c["mode"], c["K"])
    out = np.empty((S, rows - 1, 2), NF)
    out[..., 0], out[..., 1] = 1.0, NF(float(NF(c["g"])) - 1.0)
    for sd in range(S):
        tc, d = G._apg_terms(x[sd:sd + 1], eps[sd * rows:(sd + 1) * rows], NF(prm[1]), NF(prm[2]), lowp_of(c["dt"]))
        for r in range(used):
            A, B, _s = G.apg_finalise(partition_sums(tc[r], d[r]), c["g"], c["eta"], c["R"])
            out[sd, r] = NF(A), NF(B)
    return out


def ulps(a, b):
    a, b = np.ascontiguousarray(a, NF).reshape(-1), np.ascontiguousarray(b, NF).reshape(-1)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the step entry
FORMS = ("ddim", "ms")                         # x0_prev NULL: the DDIM layout and move; else the multistep layout and move
# multistep move: (cx, c0, c1, is_last) of a first-order step, a second-order step, the last step
ORDERS = {"first": (0.8125, 0.3217, 0.0, 0), "second": (0.8125, 0.4021, -0.0804, 0), "last": (0.0, 1.0, 0.0, 1)}


def step_forms():
    """(form, mode, noise) of every kernel the entry has: DDIM x three modes and 2M x two, each of FUSION / PLAIN with noise too"""
    out = [("ddim", m, False) for m in MODES] + [("ms", m, False) for m in MODES[:2]]
    return out + [(f, m, True) for f in FORMS for m in MODES[:2]]


class Case:
    """one launch of tmix_fused_tweedie_step_apg_dev: `seeds` x [4, h, w], eps [seeds * rows, 4, h, w], coefficients drawn at random (A in
    [0.5, 1.2], B in [-2, 8]), masks per seed or shared, every seed its own key.  order: "step" | "last" (DDIM) or a key of ORDERS (2M)."""

    def __init__(self, form, mode, dt, noise=False, K=3, seeds=2, h=17, w=19, order=None, shared=False, rows=None, seed=0):
        import torch
        rng = np.random.RandomState(3000 + seed + 7 * K + 131 * seeds + h)
        self.form, self.mode, self.dt, self.nz, self.K, self.seeds, self.h, self.w, self.shared = form, mode, dt, noise, K, seeds, h, w, shared
        self.ms = form == "ms"
        self.order = order or ("second" if self.ms else "step")
        self.rows = rows if rows is not None else used_rows(mode, K) + 1
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = lowp_of(dt)
        self.x = rng.randn(seeds, 4, h, w).astype(NF)
        self.prev = rng.randn(seeds, 4, h, w).astype(NF)
        self.eps_t = torch.from_numpy(rng.randn(seeds * self.rows, 4, h, w).astype(NF)).to(torch_dtype(dt))
        self.eps = self.eps_t.float().numpy()
        self.masks = rng.rand(1 if shared else seeds, K, 1, h, w).astype(NF)
        self.ab = np.stack([0.5 + 0.7 * rng.rand(seeds, self.rows - 1), -2.0 + 10.0 * rng.rand(seeds, self.rows - 1)], axis=-1).astype(NF)
        sa, s1 = sa_s1(0.2345)
        if self.ms:      # {t, sa, s1, cx, c0, c1, is_last, g}
            cx, c0, c1, last = ORDERS[self.order]
            vals = [781.0, sa, s1, cx, c0, c1, float(last), 7.5]
        else:            # {t, sa, s1, sa_next, s1_next, is_last, g, -}
            vals = [781.0, sa, s1, 0.7071, 0.6123, float(self.order == "last"), 7.5, 0.0]
        if self.nz:
            vals += [0.3125, 7.0, 0.0, 0.0]
        self.params = [float(NF(v)) for v in vals]
        self.seed_values = [SEEDS64[i % 3] + i // 3 for i in range(seeds)]

    def cuda(self):
        import torch
        from tweediemix_amd import ops
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.prev_t, self.ab_t, self.eps_d = c(self.x), c(self.masks), c(self.prev), c(self.ab), self.eps_t.cuda()
        self.prm = torch.tensor(self.params, dtype=torch.float32).cuda()
        self.keys_t = ops.noise_keys(self.seed_values, "cuda") if self.nz else None
        return self

    def launch(self, out_x, out_x0, prev, x=None, eps=None, masks=None, prm=None, ab="own", keys="own", seeds=None, rows=None, mode=None, K=None, dt=None,
               hw=None, C=4, w=None, n_win=1, yx=None, canvas=(0, 0), ms=None):
        """raw ABI call; every argument defaults to the case's own.  Returns the code."""
        import ctypes as CT
        import torch
        from tweediemix_amd import lib as L
        if yx is not None:
            yx = (CT.c_int32 * len(yx))(*yx)
        ms = self.ms if ms is None else ms
        head = [_p(self.x_t if x is None else x), _p(self.eps_d if eps is None else eps), {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[self.dt] if dt is None else dt,
                _p(self.m_t if masks is None else masks), 0 if self.shared else self.K * self.hw, _p(out_x), _p(out_x0), self.K if K is None else K, C,
                self.hw if hw is None else hw, mode_id(self.mode) if mode is None else mode, self.rows if rows is None else rows,
                self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm)]
        return L.load().tmix_fused_tweedie_step_apg_dev(*head, _p(prev) if ms else None, _p(self.ab_t) if isinstance(ab, str) else _p(ab),
                                                        _p(self.keys_t) if isinstance(keys, str) else _p(keys), self.w if w is None else w, n_win, yx,
                                                        canvas[0], canvas[1], torch.cuda.current_stream().cuda_stream)

    def run(self, **kw):
        import torch
        out_x, out_x0, prev = torch.empty_like(self.x_t), torch.empty_like(self.x_t), self.prev_t.clone()
        assert self.launch(out_x, out_x0, prev, **kw) == 0
        torch.cuda.synchronize()
        return out_x, out_x0, prev

    def reference(self):
        """(out_x, x0) of every seed from guidance.apg_step_reference / apg_multistep_reference"""
        from tweediemix_amd import guidance as G, noise as NZ
        ox, o0 = [], []
        for sd in range(self.seeds):
            x, e, m = self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows], self.masks[0 if self.shared else sd]
            key = NZ.seed_key(self.seed_values[sd]) if self.nz else None
            if self.ms:
                a, b = G.apg_multistep_reference(mode_id(self.mode), x, e, m, self.prev[sd:sd + 1], self.ab[sd], self.params, key, None, self.lowp)
            else:
                a, b = G.apg_step_reference(mode_id(self.mode), x, e, m, self.K, self.ab[sd], self.params, key, None, self.lowp)
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self):
        out_x, out_x0, prev = self.run()
        ref, ref0 = self.reference()
        what = (self.form, self.mode, self.dt, self.nz, self.K, self.seeds, self.h, self.w, self.order, self.shared)
        assert ref.dtype == NF and ref0.dtype == NF
        assert np.array_equal(out_x.cpu().numpy(), ref), what
        assert np.array_equal(out_x0.cpu().numpy(), ref0), what
        assert np.array_equal(prev.cpu().numpy(), ref0 if self.ms else self.prev), what
