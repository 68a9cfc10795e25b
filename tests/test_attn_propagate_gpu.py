"""GPU: token maps through self-attention.  tmix_sattn_propagate against an fp64 torch restatement (softmax per head, einsum with
src) on the same bf16 Q and K -- tile edges, strided views and poisoned padding, a running maximum that every key tile raises,
accumulate / overwrite / out_scale exactness, determinism and row independence, a planted partial response that comes back as the
whole rectangle -- then the propagate plan against the fp32 oracle's attn1 probabilities, the launch lists of plans without the
option, the sampler option (graphs, co-batched seeds) and the CLI end to end.

The bound of the value tests is derived, not measured: the probabilities and src each enter the second product rounded to bf16 (unit
round-off 2^-9), the fp32 sum that normalises is exact to fp32, and every head's probabilities sum to 1.  So
|err| <= 2^-7 * out_scale * H * max|src| for any src, and for non-negative src every element is within 2^-7 relative."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
TOL = 2.0 ** -7


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def ref_prop(q, k, src, H, rows, scale=0.125, out_scale=1.0):
    """fp64 torch: out_scale * sum_h softmax(q_h k_h^T scale) @ src^T for the selected batch rows -> [n_rows, n_tok, S] (fp64)"""
    out = []
    S = q.shape[1]
    for i, b in enumerate(rows):
        qh = q[b].double()[:, :H * 64].reshape(S, H, 64).transpose(0, 1)                   # [H, S, 64]
        kh = k[b].double()[:, :H * 64].reshape(S, H, 64).transpose(0, 1)
        acc = torch.zeros(src.shape[1], S, dtype=torch.float64, device=q.device)
        for h in range(H):                                                                 # one [S, S] matrix at a time
            p = torch.softmax(qh[h] @ kh[h].transpose(0, 1) * scale, dim=-1)
            acc += torch.einsum("st,jt->js", p, src[i].double())
        out.append(out_scale * acc)
    return torch.stack(out)


def check(got, want, H, out_scale, src_max, what):
    err = (got.double() - want).abs().max().item()
    rel = ((got.double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max abs err {err:.3g} (bound {TOL * abs(out_scale) * H * src_max:.3g}), max rel err {rel:.3g} (bound {TOL:.3g})")
    assert err <= TOL * abs(out_scale) * H * src_max, (what, err)
    assert rel <= TOL, (what, rel)


def _qk(B, S, C, g, mul=2.0):
    q = (torch.randn(B, S, C, device="cuda", generator=g) * mul).to(BF)
    k = (torch.randn(B, S, C, device="cuda", generator=g) * mul).to(BF)
    return q, k


# ------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("B,S,C,n_tok,rows", [
    (2, 16, 128, 1, (0, 1, None)),           # fewer keys and queries than one tile
    (3, 45, 192, 3, (0, 1, None)),           # S is no multiple of any tile; H < 4 waves
    (3, 1024, 320, 8, (1, 2, None)),         # heads are no multiple of 4; a strided row selection
    (2, 1024, 1280, 9, (0, 1, None)),        # n_tok just past 8
    (2, 4096, 128, 32, (0, 1, None)),        # 128 key tiles; the full token count
])
def test_kernel_matches_fp64_torch(B, S, C, n_tok, rows):
    need_gpu()
    from tweediemix_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B * S + C + n_tok)
    H = C // 64
    q, k = _qk(B, S, C, g)
    sel = list(range(rows[0], B, rows[1]))
    src = torch.rand(len(sel), n_tok, S, device="cuda", generator=g)
    got = ops.sattn_propagate(q, k, src, H, rows=rows)
    assert got.shape == (len(sel), n_tok, S) and got.dtype == torch.float32
    check(got, ref_prop(q, k, src, H, sel), H, 1.0, 1.0, f"B={B} S={S} H={H} n_tok={n_tok} rows={sel}")


# ------------------------------------------------------------------------------------------------ 2. views and padding
@pytest.mark.parametrize("S,off", [(45, 6), (64, 6), (64, 8), (100, 4)])
def test_views_and_poisoned_padding(S, off):
    """Q and K are the two halves of one [B, S + 19, 2C] buffer as in a plan; the rows behind S hold 100 in K (they would win every
    softmax) and the fp32 src / dst sit inside NaN guard bands at an offset of `off` floats (6: 8-byte but not 16-byte aligned)"""
    need_gpu()
    from tweediemix_amd import ops
    g = torch.Generator(device="cuda").manual_seed(S + off)
    B, C, H, n_tok, pad = 2, 192, 3, 5, 19
    q, k = _qk(B, S, C, g)
    src = torch.rand(B, n_tok, S, device="cuda", generator=g)
    want = ops.sattn_propagate(q, k, src, H)
    check(want, ref_prop(q, k, src, H, [0, 1]), H, 1.0, 1.0, f"S={S} compact")
    buf = torch.full((B, S + pad, 2 * C), 100.0, device="cuda", dtype=BF)
    buf[:, :S, :C], buf[:, :S, C:] = q, k
    n = B * n_tok * S
    flat_s = torch.full((n + 64,), float("nan"), device="cuda")
    flat_d = torch.full((n + 64,), float("nan"), device="cuda")
    sv, dv = flat_s[off:off + n].view(B, n_tok, S), flat_d[off:off + n].view(B, n_tok, S)
    sv.copy_(src)
    dv.zero_()
    got = ops.sattn_propagate(buf[:, :S, :C], buf[:, :S, C:], sv, H, out=dv)
    assert torch.equal(got, want)
    for f in (flat_s, flat_d):
        assert torch.isnan(f[:off]).all() and torch.isnan(f[off + n:]).all()              # guard bands untouched
    assert torch.equal(sv, src) and (buf[:, S:] == 100).all()


# ------------------------------------------------------------------------------------------------ 3. online softmax
def test_every_key_tile_raises_the_running_maximum():
    """Q and K times 8, and on top a ramp along the keys (one column per head: q = 32, k = 640 * key tile, 2560 logit units per tile
    against random logits of +-1000) so that every tile of 32 keys moves the running maximum and the accumulator is rescaled at each;
    the last tile is partial (269 keys) and holds the winners.  src = 1 comes back as 1."""
    need_gpu()
    from tweediemix_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    B, S, C, H, n_tok = 2, 269, 320, 5, 4
    q, k = _qk(B, S, C, g, mul=16.0)
    tile = (torch.arange(S, device="cuda") // 32).to(torch.float32)
    for h in range(H):
        q[:, :, 64 * h] = 32.0
        k[:, :, 64 * h] = (640.0 * tile).to(BF)
    src = torch.rand(B, n_tok, S, device="cuda", generator=g)
    got = ops.sattn_propagate(q, k, src, H)
    check(got, ref_prop(q, k, src, H, [0, 1]), H, 1.0, 1.0, "ramp over 9 key tiles")
    q2, k2 = _qk(B, S, C, g, mul=16.0)                    # the same scale without the ramp: the maximum moves at random tiles
    got2 = ops.sattn_propagate(q2, k2, src, H)
    check(got2, ref_prop(q2, k2, src, H, [0, 1]), H, 1.0, 1.0, "Q, K times 8")
    for qq, kk in ((q, k), (q2, k2)):
        ones = ops.sattn_propagate(qq, kk, torch.ones_like(src), H, out_scale=1.0 / H)
        d = (ones - 1).abs().max().item()
        print(f"src = 1: max |out - 1| = {d:.3g}")
        assert d <= TOL


# ------------------------------------------------------------------------------------------------ 4. accumulate and overwrite
def test_accumulate_overwrite_and_out_scale_are_exact():
    need_gpu()
    from tweediemix_amd import ops
    g = torch.Generator(device="cuda").manual_seed(6)
    B, S, C, H, n_tok = 2, 77, 256, 4, 3
    q, k = _qk(B, S, C, g)
    src = torch.rand(B, n_tok, S, device="cuda", generator=g)
    got = ops.sattn_propagate(q, k, src, H)
    again = ops.sattn_propagate(q, k, src, H, out=got.clone(), accumulate=True)
    assert torch.equal(again, got + got)
    over = ops.sattn_propagate(q, k, src, H, out=torch.full_like(got, 7.0))
    assert torch.equal(over, got)
    quarter = ops.sattn_propagate(q, k, src, H, out_scale=0.25)
    assert torch.equal(quarter, got * 0.25)
    with pytest.raises(Exception, match="overlap"):
        ops.sattn_propagate(q, k, src, H, out=src)


# ------------------------------------------------------------------------------------------------ 5. determinism, row independence
def test_kernel_is_deterministic_and_rows_are_independent():
    need_gpu()
    from tweediemix_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k = _qk(4, 1024, 320, g)
    src = torch.rand(2, 6, 1024, device="cuda", generator=g)
    a = ops.sattn_propagate(q, k, src, 5, rows=(1, 2, None))
    b = ops.sattn_propagate(q, k, src, 5, rows=(1, 2, None))
    assert torch.equal(a, b)
    one = ops.sattn_propagate(q[:2].clone(), k[:2].clone(), src[0:1].clone(), 5, rows=(1, 2, None))
    two = ops.sattn_propagate(q[2:].clone(), k[2:].clone(), src[1:2].clone(), 5, rows=(1, 2, None))
    assert torch.equal(a[0], one[0]) and torch.equal(a[1], two[0])


# ------------------------------------------------------------------------------------------------ 6. planted case
def test_planted_partial_response_comes_back_as_the_whole_rectangle():
    """a 32 x 32 grid with two rectangles whose pixels attend to each other (q = k = 6 on one column per segment and head); the raw
    map is strong on the left half of each rectangle, 0.3 on the right half, speckle elsewhere.  Thresholding the raw map loses the
    right halves; one propagation returns both rectangles exactly, and a second one still does."""
    need_gpu()
    from tweediemix_amd import masks as M, ops
    gh = gw = 32
    H = 4
    rects = [(3, 12, 5, 20), (18, 30, 10, 28)]                # y0, y1, x0, x1
    gen = torch.Generator().manual_seed(0)
    seg = torch.zeros(gh, gw, dtype=torch.long)
    for j, (y0, y1, x0, x1) in enumerate(rects):
        seg[y0:y1, x0:x1] = j + 1
    seg = seg.flatten()
    q = torch.randn(1, gh * gw, H * 64, generator=gen) * 0.1
    k = torch.randn(1, gh * gw, H * 64, generator=gen) * 0.1
    s = torch.arange(gh * gw)
    for h in range(H):
        q[0, s, 64 * h + seg] = 6.0
        k[0, s, 64 * h + seg] = 6.0
    src = 0.05 * torch.rand(2, gh, gw, generator=gen)
    for j, (y0, y1, x0, x1) in enumerate(rects):
        xm = (x0 + x1) // 2
        src[j, y0:y1, x0:xm] += 1.0
        src[j, y0:y1, xm:x1] += 0.3
    want = torch.zeros(2, gh, gw)
    for j, (y0, y1, x0, x1) in enumerate(rects):
        want[j, y0:y1, x0:x1] = 1

    def rectangles(m):
        imgs = M.attention_masks({2: m.reshape(2, gh, gw).cpu().numpy()}, [[0], [1]], gh * 8, gw * 8)
        return M.build_masks(imgs, gh, gw, "cpu")[:2, 0]
    raw = rectangles(src)
    print("raw rectangles:", [int(raw[j].sum()) for j in range(2)], "planted:", [int(want[j].sum()) for j in range(2)])
    assert not torch.equal(raw[0], want[0]) and not torch.equal(raw[1], want[1])
    qd, kd = q.to(BF).cuda(), k.to(BF).cuda()
    one = ops.sattn_propagate(qd, kd, src.reshape(1, 2, -1).cuda(), H, out_scale=1.0 / H)
    grid = one[0].cpu().reshape(2, gh, gw)
    print(f"after one round: in-rectangle {float(grid[want > 0].min()):.3f} .. {float(grid[want > 0].max()):.3f}, "
          f"background max {float(grid[want == 0].max()):.3f}")
    assert torch.equal(rectangles(one[0]), want)
    two = ops.sattn_propagate(qd, kd, one, H, out_scale=1.0 / H)
    assert torch.equal(rectangles(two[0]), want)


# ------------------------------------------------------------------------------------------------ 7. plan
def _recording_oracle(base):
    """UNetOracle whose attn1 also records, per grid size, the conditional row's probabilities of every head applied to src[S]
    ([n_tok, S] fp32), summed over heads and modules (the caller divides by heads * modules), and counts the modules"""
    from oracle import unet_oracle as UO

    class Recording(UO.UNetOracle):
        row, src, maps, sites, heads = 1, None, None, None, None

        def _attn(self, x, ehs, name, routed):
            out = super()._attn(x, ehs, name, routed)
            S = x.shape[1]
            if ehs is None and S in self.src:
                H = x.shape[-1] // self.cfg.head_dim
                q = self._lin(x[self.row:self.row + 1], name + ".to_q")[0]
                k = self._lin(x[self.row:self.row + 1], name + ".to_k")[0]
                qh = q.view(-1, H, 64).transpose(0, 1)
                kh = k.view(-1, H, 64).transpose(0, 1)
                p = torch.softmax(qh @ kh.transpose(1, 2) * self.cfg.head_dim ** -0.5, dim=-1)          # [H, S, S]
                m = torch.einsum("hst,jt->js", p.float(), self.src[S].to(p.device).float()).cpu()
                self.maps[S] = self.maps.get(S, 0) + m
                self.sites[S] = self.sites.get(S, 0) + 1
                self.heads[S] = H
            return out

    rec = Recording.__new__(Recording)
    rec.__dict__.update(base.__dict__)
    rec.maps, rec.sites, rec.heads, rec.src = {}, {}, {}, {}
    return rec


def _names(p):
    return [getattr(fn, "__name__", "") for fn, _a in p.ops]


def _tiny_plan_inputs():
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    W = U.UNetWeights(cfg, sd, "cuda")
    g = torch.Generator().manual_seed(1)
    ehs = torch.randn(2, 77, cfg.cross_dim, generator=g).to(BF).float()
    pooled = torch.randn(2, cfg.pooled_dim, generator=g)
    tid = torch.tensor([[128, 128, 0, 0, 128, 128]] * 2, dtype=torch.float32)
    return cfg, sd, W, ehs, pooled, tid


# rel L2 of prop_dst against the fp32 oracle, per level, as measured on an MI355X (printed by the test); asserted at twice that,
# rounded up to one digit, and never above the 2e-2 this project allows a plan against its oracle
PLAN_REL_MEASURED = {1: 4.28e-4, 2: 2.75e-4}
PLAN_REL_BOUND = {1: 9e-4, 2: 6e-4}


def test_propagate_plan_matches_the_oracle_tiny():
    need_gpu()
    from oracle import unet_oracle as UO
    from tweediemix_amd import unet as U
    cfg, sd, W, ehs, pooled, tid = _tiny_plan_inputs()
    h = w = 16
    spec = U.TokenPropSpec(3, row0=1, row_step=2, n_rows=1)
    plan = U.UNetPlan(W, 2, h, w, U.KVCache(W, ehs, [0, 0]), pooled, tid, token_prop=spec)
    assert sorted(plan.prop_src) == sorted(plan.prop_dst) == list(U.attention_levels(cfg))
    g = torch.Generator().manual_seed(4)
    for lvl, s in plan.prop_src.items():
        assert s.shape == plan.prop_dst[lvl].shape == (1, 3, (h >> lvl) * (w >> lvl)) and float(plan.prop_dst[lvl].abs().max()) == 0.0
        s.copy_(torch.rand(s.shape, generator=g))
    x = torch.randn(1, 4, h, w, generator=g).repeat(2, 1, 1, 1)
    eps = plan(x.cuda(), 601).float().cpu()
    torch.cuda.synchronize()
    rec = _recording_oracle(UO.UNetOracle(UO.TINY, sd))
    rec.src = {(h >> lvl) * (w >> lvl): s[0].cpu() for lvl, s in plan.prop_src.items()}
    dev = next(iter(rec.sd.values())).device
    ref = rec.forward(x.to(dev), 601, ehs.to(dev), pooled.to(dev), tid.to(dev)).float().cpu()
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    assert rel(eps, ref) <= 2e-2
    for lvl, d in plan.prop_dst.items():
        S = (h >> lvl) * (w >> lvl)
        want = rec.maps[S] / (rec.heads[S] * rec.sites[S])
        r = rel(d[0].cpu(), want)
        print(f"tiny propagate plan, level {lvl}: {rec.sites[S]} attn1 sites x {rec.heads[S]} heads, rel L2 {r:.3g} "
              f"(bound {PLAN_REL_BOUND[lvl]:.0e})")
        assert rec.sites[S] == plan._prop_sites[lvl]
        assert r <= PLAN_REL_BOUND[lvl] <= 2e-2, (lvl, r)
    # a constant map comes back as that constant: the launches of a level sum to the mean over heads and modules of a stochastic matrix
    for lvl, s in plan.prop_src.items():
        s.fill_(0.75)
        plan.prop_dst[lvl].zero_()
    plan(x.cuda(), 601)
    for lvl, d in plan.prop_dst.items():
        assert (d - 0.75).abs().max().item() <= 0.75 * TOL, lvl


def test_launch_lists_without_the_option_are_unchanged():
    """the propagate plan is the plain plan plus one tmix_sattn_propagate behind every attn1 launch of a probed level; a plan without
    token_prop and the probe plan record the launch lists written down from the commit before the feature (tests/golden)"""
    need_gpu()
    from tweediemix_amd import unet as U
    cfg, sd, W, ehs, pooled, tid = _tiny_plan_inputs()
    mk = lambda **kw: U.UNetPlan(W, 2, 16, 16, U.KVCache(W, ehs, [0, 0]), pooled, tid, autotune=False, **kw)
    plain, prop = mk(), mk(token_prop=U.TokenPropSpec(3))
    probe = mk(token_maps=U.TokenMapSpec((4, 7, 9), row0=1, row_step=2, n_rows=1))
    one_level = mk(token_prop=U.TokenPropSpec(3, levels=(2,)))
    n_attn1 = len(U.attention_blocks(cfg))
    assert plain.prop_spec is None and not plain.prop_src and not plain.prop_dst and not probe.prop_dst
    assert "tmix_sattn_propagate" not in _names(plain) and "tmix_sattn_propagate" not in _names(probe)
    assert [n for n in _names(prop) if n != "tmix_sattn_propagate"] == _names(plain)
    assert _names(prop).count("tmix_sattn_propagate") == n_attn1 == 17 == sum(prop._prop_sites.values())
    assert _names(one_level).count("tmix_sattn_propagate") == one_level._prop_sites[2] < n_attn1
    for i, n in enumerate(_names(prop)):                  # each one directly behind an attention launch
        if n == "tmix_sattn_propagate":
            assert _names(prop)[i - 1].startswith("tmix_attn_fwd"), _names(prop)[i - 1]
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_launches_tiny16.json")))
    assert _names(plain) == gold["plain"] and _names(probe) == gold["probe"]


# ------------------------------------------------------------------------------------------------ 8. sampler and CLI
def _tiny(kind, K=3):
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, kind, K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, 77, cfg.cross_dim, generator=g).to(BF).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, 77, cfg.cross_dim, generator=g).to(BF).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", (kind, con)), te, ts


def _cfg(S, h, w, jumping=2):
    return S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=jumping,
                         resolution_h=h * 8, resolution_w=w * 8)


def _no_provider(x0):
    raise AssertionError("the mask provider must not be called with attention_masks")


def test_sampler_propagate_option(monkeypatch):
    """propagate=0 is the run without the key, bit for bit; propagate=1 exposes propagated_maps, replays the propagate plan once on
    the last look-ahead call's timestep, changes the final latent only through the masks, and gives the same bits with graphs on and off"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    W, te, ts = _tiny("custom", K)
    cfg = _cfg(S, h, w)
    xT = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(7))

    def run(am, graphs, provider=_no_provider):
        tw = S.Tweediemix(cfg, W, te, ts, provider, concept_num=K, use_graphs=graphs, attention_masks=am)
        return tw.run_fusion(xT.clone()).cpu(), tw
    base = dict(tokens=[[4], [7, 9]], threshold=0.5)
    lat_n, tw_n = run(base, True)
    lat_0, tw_0 = run(dict(base, propagate=0), True)
    assert torch.equal(lat_0, lat_n) and torch.equal(tw_0.masks, tw_n.masks) and tw_0.propagated_maps is None
    for lvl, m in tw_n.attention_maps[0].items():
        assert np.array_equal(tw_0.attention_maps[0][lvl], m)
    assert "propagate" not in tw_0.plans and [c[0] for c in tw_0.unet_calls] == [c[0] for c in tw_n.unet_calls]

    lat_g, tw_g = run(dict(base, propagate=1), True)
    lat_e, tw_e = run(dict(base, propagate=1), False)
    for tw in (tw_g, tw_e):
        assert sorted(tw.propagated_maps[0]) == [1, 2] and tw.propagated_maps[0][2].shape == (3, 4, 4)
        assert all(np.isfinite(m).all() and m.min() >= 0 for m in tw.propagated_maps[0].values())
        kinds = [c[0] for c in tw.unet_calls]
        assert kinds.count("probe") == cfg.jumping_steps and kinds.count("propagate") == 1
        i = kinds.index("propagate")
        assert kinds[i - 1] == "probe" and tw.unet_calls[i][2] == tw.unet_calls[i - 1][2]            # the last look-ahead call's timestep
        for lvl, m in tw_n.attention_maps[0].items():
            assert np.array_equal(tw.attention_maps[0][lvl], m)                                      # the raw maps stay what they were
        ms = tw.masks.cpu()
        assert ms.shape == (K, 1, h, w) and set(torch.unique(ms).tolist()) <= {0.0, 1.0}
        assert torch.equal(ms[K - 1], torch.clamp(1 - ms[:K - 1].sum(0), min=0))
    assert torch.equal(lat_g, lat_e) and torch.equal(tw_g.masks, tw_e.masks)                          # graphs on and off agree
    for lvl, m in tw_g.propagated_maps[0].items():
        assert np.array_equal(tw_e.propagated_maps[0][lvl], m)
        raw = tw_g.attention_maps[0][lvl]
        # mean over heads and modules of a stochastic matrix: every propagated value lies between the raw map's extremes
        assert m.min() >= raw.min() * (1 - TOL) - 1e-30 and m.max() <= raw.max() * (1 + TOL)
    # the rounds touch nothing but the masks: a normal run handed these masks ends in the identical latent
    ms = tw_g.masks.clone()
    lat_fixed, fixed = run(None, True, provider=lambda x0: ms)
    assert torch.equal(lat_fixed, lat_g) and "propagate" not in fixed.plans
    # two rounds: the propagate plan twice, on the same timestep
    _lat2, tw2 = run(dict(base, propagate=2), True)
    assert [c[0] for c in tw2.unet_calls].count("propagate") == 2


def test_sampler_propagate_co_batched_seeds_match_single_runs(monkeypatch):
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    W, te, ts = _tiny("custom", K)
    cfg = _cfg(S, h, w)
    am = dict(tokens=[[4], [7]], propagate=1)
    xT = torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(8))
    singles = []
    for i in range(2):
        tw = S.Tweediemix(cfg, W, te, ts, _no_provider, concept_num=K, attention_masks=am)
        singles.append((tw.run_fusion(xT[i:i + 1].clone()).cpu(), tw.masks.clone().cpu(), tw.propagated_maps[0]))
    tw2 = S.Tweediemix(cfg, W, te, ts, _no_provider, concept_num=K, attention_masks=am, n_seeds=2, use_graphs=True)
    both = tw2.run_fusion(xT.clone()).cpu()
    assert tw2.masks.shape == (2, K, 1, h, w) and tw2.plan("propagate").B == 4 and len(tw2.propagated_maps) == 2
    for i in range(2):
        assert torch.equal(tw2.masks[i].cpu(), singles[i][1]), i
        for lvl, m in singles[i][2].items():
            d = np.abs(tw2.propagated_maps[i][lvl] - m).max() / np.abs(m).max()
            print(f"seed {i} level {lvl}: co-batched propagated maps vs single run, max rel diff {d:.3g}")
            assert d <= 1e-3, (i, lvl, d)
        assert (both[i:i + 1] - singles[i][0]).abs().max().item() <= 1e-3, i      # test_sampler_gpu.py's bound for co-batched seeds


def test_cli_attn_mask_propagate_end_to_end(tmp_path):
    need_gpu()
    spec = importlib.util.spec_from_file_location("fs_cli_prop_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    out = tmp_path / "out"
    argv = ["--tiny", "--synthetic", "--mask_source", "attention", "--attn_mask_propagate", "1", "--save_attention_maps",
            "--mask_token_ids", "4+7", "--seed", "9", "--prompt", "a cat+a dog+a mountain", "--prompt_orig", "cat and dog",
            "--concepts", "cat+dog+mountain", "--modifier_token", "<new1>+<new2>+<new3>", "--seg_concepts", "a cat+a dog",
            "--guidance_scale", "0.8", "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "2",
            "--resolution_h", "128", "--resolution_w", "128", "--output_path", str(out), "--output_path_all", str(out / "all")]
    lat = fs.main(argv)
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all()
    from PIL import Image
    for name in ("a cat", "a dog"):
        im = np.array(Image.open(out / f"{name}.jpg").convert("L"))
        assert im.shape == (128, 128) and im.max() > 128
    for lvl, side in ((1, 8), (2, 4)):
        raw = np.load(out / f"attention_maps_9_level{lvl}.npy")
        prop = np.load(out / f"attention_maps_9_level{lvl}_prop.npy")
        assert raw.shape == prop.shape == (2, side, side) and np.isfinite(prop).all() and not np.array_equal(raw, prop)
