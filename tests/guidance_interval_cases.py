"""Shared by tests/test_guidance_interval_cpu.py and tests/test_guidance_interval_gpu.py: the inputs of one launch of
tmix_fused_tweedie_step_cond_dev with their restatement, the stand-in UNet of the sampler tests and the fp32 loop restatement of a whole
stand-in trajectory.  Nothing here touches the GPU at import."""
import numpy as np

NF = np.float32
MODES = ("fusion", "plain")
FORMS = ("ddim", "ms1", "ms2")               # the DDIM move; the multistep move, first order (c1 == 0) and second order
NOISES = ("none", "cz", "last")              # keys NULL; keys with cz != 0; keys with cz != 0 on the last step (cz is not applied)
SEEDS64 = (182, (0x9E3779B9 << 32) + 7, 0xFFFFFFFFFFFFFFFF)
STEP_FUSION, STEP_PLAIN, STEP_RESAMPLE = 0, 1, 2


def mode_id(name):
    return {"fusion": STEP_FUSION, "plain": STEP_PLAIN, "resample": STEP_RESAMPLE}[name]


def torch_dtype(dt):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]


def _p(t):
    return None if t is None else t.data_ptr()


class Case:
    """one launch of the unguided entry: `seeds` x [4, h, w], eps [seeds * rows, 4, h, w] WITHOUT an unconditional row, masks per seed or shared,
    every seed its own key.  Host arrays are built at construction, device tensors by cuda()."""

    def __init__(self, mode, dt, form="ddim", noise="none", K=3, seeds=2, h=17, w=19, shared_masks=False, rows=None, seed=0, g_slot=0.8):
        import torch
        rng = np.random.RandomState(1000 + seed + 7 * K + 131 * seeds + h)
        self.mode, self.dt, self.form, self.noise, self.K, self.seeds, self.h, self.w = mode, dt, form, noise, K, seeds, h, w
        self.ms, self.nz = form != "ddim", noise != "none"
        self.rows = rows if rows is not None else (1 if mode == "plain" else K)
        self.n, self.hw = 4 * h * w, h * w
        self.lowp = np.float16 if dt == "f16" else None
        self.x = rng.randn(seeds, 4, h, w).astype(NF)
        self.prev = rng.randn(seeds, 4, h, w).astype(NF)
        self.eps_t = torch.from_numpy(rng.randn(seeds * self.rows, 4, h, w).astype(NF)).to(torch_dtype(dt))
        self.eps = self.eps_t.float().numpy()                        # fp32 copies of values of the eps dtype
        self.masks = rng.rand(1 if shared_masks else seeds, K, 1, h, w).astype(NF)
        self.shared = shared_masks
        sa, s1 = float(np.sqrt(NF(0.2345))), float(np.sqrt(NF(1) - NF(0.2345)))
        is_last = 1.0 if noise == "last" else 0.0
        if self.ms:      # {t, sa, s1, cx, c0, c1, is_last, g}
            move = [0.8125, 0.4021, -0.0804 if form == "ms2" else 0.0, is_last, g_slot]
        else:            # {t, sa, s1, sa_next, s1_next, is_last, g, -}
            move = [0.7071, 0.6123, is_last, g_slot, 0.0]
        vals = [781.0, sa, s1] + move
        if self.nz:
            vals += [0.3125, 7.0, 0.0, 0.0]
        self.params = [float(NF(v)) for v in vals]                   # the fp32 values the kernel reads
        self.seed_values = [SEEDS64[i % 3] + i // 3 for i in range(seeds)]

    def cuda(self):
        import torch
        from tweediemix_amd import ops
        c = lambda a: torch.from_numpy(a).cuda()
        self.x_t, self.m_t, self.prev_t, self.eps_d = c(self.x), c(self.masks), c(self.prev), self.eps_t.cuda()
        self.prm = torch.tensor(self.params, dtype=torch.float32).cuda()
        self.keys_t = ops.noise_keys(self.seed_values, "cuda") if self.nz else None
        return self

    def head(self, out_x, out_x0, x=None, eps=None, masks=None, prm=None, seeds=None, rows=None, mode=None, K=None, dt=None, hw=None, C=4, mss=None):
        from tweediemix_amd import lib as L
        if mss is None:
            mss = 0 if self.shared else self.K * self.hw
        return [_p(self.x_t if x is None else x), _p(self.eps_d if eps is None else eps), {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}[self.dt] if dt is None else dt,
                _p(self.m_t if masks is None else masks), mss, _p(out_x), _p(out_x0), self.K if K is None else K, C,
                self.hw if hw is None else hw, mode_id(self.mode) if mode is None else mode, self.rows if rows is None else rows,
                self.seeds if seeds is None else seeds, _p(self.prm if prm is None else prm)]

    def launch(self, out_x, out_x0, prev, keys=None, w=None, n_win=1, yx=None, canvas=(0, 0), no_keys=False, **kw):
        """raw ABI call of the entry; every argument defaults to the case's own.  Returns the code."""
        import ctypes as C
        import torch
        from tweediemix_amd import lib as L
        if yx is not None:
            yx = (C.c_int32 * len(yx))(*yx)
        keys = None if no_keys else (self.keys_t if keys is None else keys)
        return L.load().tmix_fused_tweedie_step_cond_dev(*self.head(out_x, out_x0, **kw), _p(prev) if self.ms else None, _p(keys),
                                                         self.w if w is None else w, n_win, yx, canvas[0], canvas[1],
                                                         torch.cuda.current_stream().cuda_stream)

    def run(self, **kw):
        import torch
        out_x, out_x0, prev = torch.empty_like(self.x_t), torch.empty_like(self.x_t), self.prev_t.clone()
        assert self.launch(out_x, out_x0, prev, **kw) == 0
        torch.cuda.synchronize()
        return out_x, out_x0, prev

    def reference(self):
        """(out_x, x0) of every seed from guidance.cond_step_reference; the history after the step is x0 (multistep forms) or untouched"""
        from tweediemix_amd import guidance as G, noise as NZ
        ox, o0 = [], []
        for sd in range(self.seeds):
            a, b = G.cond_step_reference(mode_id(self.mode), self.x[sd:sd + 1], self.eps[sd * self.rows:(sd + 1) * self.rows],
                                         self.masks[0 if self.shared else sd], self.prev[sd:sd + 1] if self.ms else None, self.params,
                                         NZ.seed_key(self.seed_values[sd]) if self.nz else None, None, self.lowp)
            ox.append(a)
            o0.append(b)
        return np.concatenate(ox), np.concatenate(o0)

    def check(self):
        out_x, out_x0, prev = self.run()
        ref, ref0 = self.reference()
        what = (self.mode, self.dt, self.form, self.noise, self.K, self.seeds, self.h, self.w, self.shared)
        assert ref.dtype == NF and np.array_equal(out_x.cpu().numpy(), ref), what
        assert np.array_equal(out_x0.cpu().numpy(), ref0), what
        assert np.array_equal(prev.cpu().numpy(), ref0 if self.ms else self.prev), what


# ------------------------------------------------------------------------------------------------ the sampler with a stand-in UNet
K3, H, W = 3, 16, 16
ROWS = {"fusion": K3 + 1, "fusion_base": K3 + 1, "start": K3 + 1, "plain": 2, "fusion_c": K3, "fusion_base_c": K3, "plain_c": 1}
INTERVAL = (700, 250)


class NoWeights:
    kind = "custom"
    K = K3

    def __init__(self, device):
        import torch
        self.device = torch.device(device)


def make_cfg(S, n=10, R=1, J=1, h=H, w=W, g=0.8):
    return S.make_config(guidance_scale=g, n_timesteps=n, t_cond=0.2, t_stop=0.8, resampling_steps=R, jumping_steps=J, resolution_h=h * 8,
                         resolution_w=w * 8)


def standin_eps(kind, x, t):
    """the stand-in UNet: an elementwise function of (prompt row, x, t), so a seed's eps does not depend on what it is co-batched with.  A "_c" kind
    returns its guided twin's rows without the unconditional one: the conditional rows are the same function in both."""
    import torch
    cond = kind.endswith("_c")
    rows = ROWS[kind[:-2] if cond else kind]
    e = torch.stack([torch.sin(x * (1.0 + 0.25 * r) + 0.01 * float(t) + r) for r in range(1 if cond else 0, rows)], dim=1)
    return e.reshape(-1, *x.shape[1:]).contiguous()


def standin_sampler(device, seeds=1, log=None, **kw):
    """Tweediemix on NoWeights with the stand-in attached; the stand-in appends (kind, rows, t) to unet_calls as a real plan's call does"""
    from tweediemix_amd import masks as M, sampler as S
    masks = M.build_masks(M.partition_rectangle_masks(K3, H * 8, W * 8, seed=3), H, W, device)
    cfg = kw.pop("cfg", None) or make_cfg(S)
    tw = S.Tweediemix(cfg, NoWeights(device), None, None, lambda x0: masks, concept_num=K3, n_seeds=seeds, **kw)

    def unet(kind, x, t):
        e = standin_eps(kind, x, t)
        tw.unet_calls.append((kind, e.shape[0] // x.shape[0], int(t)))
        if log is not None:
            log.append((kind, int(t), x.clone(), e.clone()))
        return e
    tw._unet = unet
    return tw, masks


def standin_eps_np(kind, x, t):
    """standin_eps in fp32 numpy"""
    cond = kind.endswith("_c")
    rows = ROWS[kind[:-2] if cond else kind]
    e = np.stack([np.sin(x * NF(1.0 + 0.25 * r) + NF(0.01 * float(t)) + NF(r), dtype=NF) for r in range(1 if cond else 0, rows)], axis=1)
    return e.reshape(-1, *x.shape[1:])


def loop_reference(xT, masks, interval, n=10, spacing="leading", solver="ddim", R=1, J=1, g=0.8, t_cond=0.2, eps_fn=standin_eps_np):
    """fp32 numpy restatement of Tweediemix.run_fusion (non-LoRA window, eta = 0, no rescale) with a guidance interval, written as the loop of
    fusion_sampling.py with the project's schedule: -> (calls [(kind, rows, t)], states [the latent after every schedule entry]).  Guided steps
    are the oracle's (oracle.tweedie_oracle) or solver.multistep_step_reference, unguided ones guidance.cond_step_reference.  xT [S, 4, h, w]."""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import guidance as G, ops, solver as SV
    from tweediemix_amd.schedule import Schedule
    sch = Schedule(n, spacing=spacing)
    ts = sch.timesteps
    ic = int(n * t_cond) if spacing == "leading" else sch.index_at_or_below(Schedule(n).timesteps[int(n * t_cond)])
    t_cond_cur, t_cond_prev, start_t = ts[ic], ts[ic - 1], ts[0]
    x = np.asarray(xT, NF).copy()
    S, K = x.shape[0], masks.shape[0]
    g = NF(g)
    calls, states = [], []
    hist, ms_last = np.zeros_like(x), None

    def unet(kind, xin, t):
        e = eps_fn(kind, xin, t)
        calls.append((kind, e.shape[0] // S, int(t)))
        return e

    def per_seed(fn, xin, eps):
        rows = eps.shape[0] // S
        return np.concatenate([fn(xin[sd:sd + 1], eps[sd * rows:(sd + 1) * rows], sd) for sd in range(S)])

    for i, t in enumerate(ts):
        nt = sch.next_t(t)
        at, an = sch.alpha(t), sch.alpha(nt)
        last = t == 1
        guided = t == start_t or interval is None or interval[1] <= t <= interval[0]
        fusion = t <= t_cond_cur
        if t == start_t:
            for _ in range(R):
                eps = unet("start", x, t)
                xd = per_seed(lambda a, e, sd: TO.fused_resample_down(a, e, K, g, at, an), x, eps)
                eps_n = unet("plain", xd, nt)
                x = per_seed(lambda a, e, sd: TO.fused_resample_up(a, e, g, at, an), xd, eps_n)
            eps = unet("start", x, t)
            x = per_seed(lambda a, e, sd: TO.fused_plain_step(a, e[:2], g, at, an, last)[0], x, eps)
            ms_last = None
        else:
            kind = ("fusion" if fusion else "plain") + ("" if guided else "_c")
            mode = STEP_FUSION if fusion else STEP_PLAIN
            m = masks if fusion else None
            eps = unet(kind, x, t)
            sa, s1, san, s1n = ops.step_coeffs(at, an)
            if solver == "ddim":
                if guided:
                    step = (lambda a, e, sd: TO.fused_fusion_step(a, e, masks, g, at, an, last)[0]) if fusion else \
                        (lambda a, e, sd: TO.fused_plain_step(a, e, g, at, an, last)[0])
                else:
                    step = lambda a, e, sd: G.cond_step_reference(mode, a, e, m, None, [t, sa, s1, san, s1n, float(last), g, 0.0])[0]
                x = per_seed(step, x, eps)
            else:
                second = ms_last == (i - 1, mode, guided)
                cx, c0, c1 = (0.0, 1.0, 0.0) if last else SV.multistep_coeffs(sch.alpha(ts[i - 1]), at, an, second)
                new_hist = np.zeros_like(x)

                def step(a, e, sd):
                    if guided:
                        o, x0 = SV.multistep_step_reference(mode, a, e, m, hist[sd:sd + 1], g, sa, s1, cx, c0, c1, last)
                    else:
                        o, x0 = G.cond_step_reference(mode, a, e, m, hist[sd:sd + 1], [t, sa, s1, cx, c0, c1, float(last), g])
                    new_hist[sd:sd + 1] = x0
                    return o
                x = per_seed(step, x, eps)
                hist, ms_last = new_hist, (i, mode, guided)
        if t == t_cond_prev:                    # the look-ahead: always guided, does not move the trajectory
            xt, tt = x, nt
            for _ in range(J):
                eps_j = unet("plain", xt, tt)
                a_t, a_n = sch.alpha(tt), sch.alpha(tt - 150)
                xt = per_seed(lambda a, e, sd: TO.fused_plain_step(a, e, g, a_t, a_n, False)[0], xt, eps_j)
                tt -= 150
        states.append(x.copy())
    return calls, states
