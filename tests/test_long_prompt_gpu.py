"""GPU: long prompts.  tmix_xattn_token_maps_long against fp32 torch (past 80 keys, past 8 positions), tmix_attn_fwd at the 154 and
231 keys of two and three chunks, the text towers on chunked prompts, UNet plans over 154 keys against the fp32 oracle, the probe
plan with positions in the second chunk, and the CLI end to end.

Measured on an MI355X (printed by the tests): tmix_xattn_token_maps_long max-abs error 4.2e-7 (H = 2, 154 keys, 9 positions),
7.2e-7 (H = 4, 231 keys, 32 positions), 1.2e-6 (H = 20, 154 keys, 12 positions), 3.0e-7 (H = 2, 81 keys, 1 position) against the
bound 1e-4 * H; tmix_attn_fwd at 154 / 231 keys at most 6.0e-3 max-abs on outputs of magnitude ~0.5."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------ 5. token maps, long form
def ref_maps(q, k, H, Lk, rows, tokens, scale=0.125):
    """fp32 torch: softmax(q k^T scale) of every head at the token columns, summed over heads -> [n_rows, n_tok, Sq]
    (the restatement of tests/test_attn_masks_gpu.py; Q rows / K rows behind Sq / Lk are never read)"""
    out = []
    for b in rows:
        qh = q[b].float().view(q.shape[1], -1)[:, :H * 64].view(-1, H, 64).transpose(0, 1)          # [H, Sq, 64]
        kh = k[b, :Lk].float()[:, :H * 64].reshape(Lk, H, 64).transpose(0, 1)                          # [H, Lk, 64]
        p = torch.softmax(qh @ kh.transpose(1, 2) * scale, dim=-1)                                    # [H, Sq, Lk]
        out.append(p[:, :, list(tokens)].sum(0).transpose(0, 1))                                       # [n_tok, Sq]
    return torch.stack(out)


def _positions(Lk, n_tok):
    """n_tok distinct positions that touch every key tile of 32, both lane halves, the first and the last key"""
    base = [0, Lk - 1, 31, 32, 63, 64, 95, 96, 127, 128, Lk - 2, 4, 36, 77, 78, 82, 100, 130, 150, 153]
    pos = [p for p in dict.fromkeys(base) if 0 <= p < Lk]
    pos += [p for p in range(Lk) if p % 7 == 3 and p not in pos]
    return pos[:n_tok]


def _qk(B, Sq, C, Lk, seed):
    """Q [B, Sq rounded up to the 32-query tile (+ one tile), C] and K [B, 240, C]: the rows behind Sq and behind Lk hold NaN"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Sp = (Sq + 31) // 32 * 32 + 32
    q = torch.full((B, Sp, C), float("nan"), device="cuda", dtype=BF)
    k = torch.full((B, 240, C), float("nan"), device="cuda", dtype=BF)
    q[:, :Sq] = (torch.randn(B, Sq, C, device="cuda", generator=g) * 2).to(BF)
    k[:, :Lk] = (torch.randn(B, Lk, C, device="cuda", generator=g) * 2).to(BF)
    return q, k


@pytest.mark.parametrize("B,Sq,C,Lk,n_tok", [(2, 16, 128, 154, 9), (2, 64, 256, 231, 32), (2, 1024, 1280, 154, 12), (2, 40, 128, 81, 1)])
def test_long_kernel_matches_fp32_torch(B, Sq, C, Lk, n_tok):
    """Bound: the project's own for the short form, 1e-4 * H max-abs (the probabilities of one query sum to at most H over the
    heads; the kernel's error is fp32 summation order and exp2 rounding).  K rows behind Lk and Q rows behind Sq are NaN."""
    need_gpu()
    from tweediemix_amd import ops
    H = C // 64
    q, k = _qk(B, Sq, C, Lk, B * Sq + C + n_tok + Lk)
    qv = q[:, :Sq]                                                # a view: the batch stride spans the NaN rows
    tok = _positions(Lk, n_tok)
    assert len(tok) == n_tok
    got = ops.xattn_token_maps(qv, k, tok, H, Lk=Lk, rows=(1, 2, None), long=True)
    want = ref_maps(q[:, :Sq], k, H, Lk, [1], tok)
    err = (got - want).abs().max().item()
    print(f"long maps B={B} Sq={Sq} C={C} Lk={Lk} n_tok={n_tok}: max abs err {err:.3g} (H = {H}, bound {1e-4 * H:.1e})")
    assert got.shape == (1, n_tok, Sq) and torch.isfinite(got).all()
    assert err <= 1e-4 * H, err
    # two calls are identical; accumulate doubles; overwrite ignores what the output held
    assert torch.equal(ops.xattn_token_maps(qv, k, tok, H, Lk=Lk, rows=(1, 2, None), long=True), got)
    again = ops.xattn_token_maps(qv, k, tok, H, Lk=Lk, rows=(1, 2, None), out=got.clone(), accumulate=True, long=True)
    assert torch.equal(again, got + got)
    over = ops.xattn_token_maps(qv, k, tok, H, Lk=Lk, rows=(1, 2, None), out=torch.full_like(got, 7.0), long=True)
    assert torch.equal(over, got)
    # every row selection form agrees with the reference too
    allr = ops.xattn_token_maps(qv, k, tok, H, Lk=Lk, rows=(0, 1, None), long=True)
    assert torch.equal(allr[1], got[0]) and (allr - ref_maps(q[:, :Sq], k, H, Lk, [0, 1], tok)).abs().max().item() <= 1e-4 * H


def test_long_kernel_rows_do_not_depend_on_the_batch():
    need_gpu()
    from tweediemix_amd import ops
    q, k = _qk(4, 200, 320, 154, 5)
    qv, tok = q[:, :200], _positions(154, 12)
    four = ops.xattn_token_maps(qv, k, tok, 5, Lk=154, rows=(1, 2, None))
    one = ops.xattn_token_maps(qv[:2].clone(), k[:2].clone(), tok, 5, Lk=154, rows=(1, 2, None))
    two = ops.xattn_token_maps(qv[2:].clone(), k[2:].clone(), tok, 5, Lk=154, rows=(1, 2, None))
    assert four.shape == (2, 12, 200) and torch.equal(four[0], one[0]) and torch.equal(four[1], two[0])


def test_long_entry_point_at_77_keys_and_8_positions_is_the_short_one_bit_for_bit():
    need_gpu()
    from tweediemix_amd import ops
    q, k = _qk(2, 1000, 1280, 77, 9)
    qv, tok = q[:, :1000], [1, 4, 7, 31, 32, 63, 64, 76]
    short = ops.xattn_token_maps(qv, k, tok, 20, Lk=77, rows=(1, 2, None), long=False)
    long = ops.xattn_token_maps(qv, k, tok, 20, Lk=77, rows=(1, 2, None), long=True)
    assert torch.isfinite(short).all() and torch.equal(short, long)
    # nine positions at 77 keys run the long kernel on three key tiles: the first eight maps agree with the short form within the bound
    nine = ops.xattn_token_maps(qv, k, tok + [76 - 3], 20, Lk=77, rows=(1, 2, None))
    assert (nine[:, :8] - short).abs().max().item() <= 1e-4 * 20
    assert (nine - ref_maps(qv, k, 20, 77, [1], tok + [73])).abs().max().item() <= 1e-4 * 20


def test_all_keys_sum_to_the_head_count():
    """32 positions at a time over all 231 keys: every head's probabilities sum to 1, so padding keys got none"""
    need_gpu()
    from tweediemix_amd import ops
    q, k = _qk(1, 45, 192, 231, 3)
    tot = 0
    for p0 in range(0, 231, 32):
        tot = tot + ops.xattn_token_maps(q[:, :45], k, list(range(p0, min(p0 + 32, 231))), 3, Lk=231).sum(1)
    assert torch.allclose(tot, torch.full_like(tot, 3.0), atol=3e-4)


def test_planted_key_in_the_second_chunk_peaks_at_the_planted_queries():
    """the planted-key case of tests/test_attn_masks_gpu.py with the key at 77 + 5 of a 154-key prompt and nine positions"""
    need_gpu()
    from tweediemix_amd import ops
    gh = gw = 32
    H, Lk = 4, 154
    tok = [4, 7, 20, 76, 77 + 5, 100, 120, 140, 153]
    j = tok.index(82)
    y0, y1, x0, x1 = 3, 12, 5, 20
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, gh * gw, H * 64, generator=g) * 0.1
    k = torch.randn(2, 160, H * 64, generator=g) * 0.1
    sel = torch.zeros(gh, gw, dtype=torch.bool)
    sel[y0:y1, x0:x1] = True
    for h in range(H):
        k[1, 82, h * 64 + 3] = 8.0
        q[1, sel.flatten(), h * 64 + 3] = 8.0
    maps = ops.xattn_token_maps(q.to(BF).cuda(), k.to(BF).cuda(), tok, H, Lk=Lk, rows=(1, 1, 1))[0].cpu()      # [9, 1024]
    m = maps[j].view(gh, gw)                       # planted logit 64 / 8 = 8 against 153 keys near 0: p = e^8 / (e^8 + 153) = 0.95 per head
    assert m[sel].min().item() > 0.5 * H and m[~sel].max().item() < 0.1 * H        # the planted key takes the planted queries
    others = torch.cat([maps[:j], maps[j + 1:]])
    assert others.max().item() < 0.1 * H


# ------------------------------------------------------------------------------------------------ 6. tmix_attn_fwd at 154 / 231 keys
def _close(out, ref, rtol=2 ** -6, atol_frac=4e-3):
    """the bound tests/test_ops_gpu.py applies to tmix_attn_fwd (its `close` with rtol 2^-6, atol 4e-3 of the largest value)"""
    out, ref = out.float(), ref.float()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    atol = atol_frac * ref.abs().max().item() + 1e-6
    err = (out - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    assert not bad.any(), f"max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g}), {int(bad.sum())} bad"
    return err.max().item()


@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("Sq", [64, 1000])
@pytest.mark.parametrize("Skv", [154, 231])
def test_attention_at_two_and_three_chunks_of_keys(Skv, Sq, H):
    """K rows behind Skv are NaN; V^T columns [Skv, ldvt) hold alternating +-3e38 (the header's "finite"), ldvt = 160 / 232 as KVCache
    pads them"""
    need_gpu()
    from tweediemix_amd import ops
    B, Cc = 2, H * 64
    g = torch.Generator(device="cuda").manual_seed(Skv + Sq + H)
    q = torch.randn(B, Sq, Cc, device="cuda", generator=g).to(BF)
    kf = torch.randn(B, Skv, Cc, device="cuda", generator=g).to(BF)
    v = torch.randn(B, Skv, Cc, device="cuda", generator=g).to(BF)
    k = torch.full((B, 240, Cc), float("nan"), device="cuda", dtype=BF)
    k[:, :Skv] = kf
    ld = (Skv + 7) // 8 * 8
    assert ld in (160, 232)
    vt = torch.where(torch.arange(ld, device="cuda") % 2 == 0, 3e38, -3e38).to(BF).expand(B, Cc, ld).contiguous()
    vt[:, :, :Skv] = v.transpose(1, 2)
    out = ops.attention(q, k, vt, H, Skv, 0.125)

    def heads(t):
        return t.float().reshape(B, -1, H, 64).transpose(1, 2)
    ref = F.scaled_dot_product_attention(heads(q), heads(kf), heads(v), scale=0.125).transpose(1, 2).reshape(B, Sq, Cc)
    err = _close(out, ref)
    print(f"attn Skv={Skv} Sq={Sq} H={H}: max abs err {err:.3g}")
    assert torch.equal(ops.attention(q, k, vt, H, Skv, 0.125), out)


# ------------------------------------------------------------------------------------------------ 7. text towers
def _rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm())


def test_text_towers_on_chunked_prompts(golden_dir):
    """a 2-chunk and a 1-chunk prompt, long=True: bit-equal to the four chunk texts as four short prompts of one batch, concatenated;
    pooled = chunk 0's; each chunk within tests/test_text_gpu.py's bounds of the fp32 text oracle (hidden 2e-2, pooled 3e-2 rel L2)"""
    need_gpu()
    from oracle import clip_oracle as CO
    from tweediemix_amd import text as T, weights as Wt
    toks = [T.ClipBPETokenizer.from_pretrained(os.path.join(golden_dir, "clip_tok")) for _ in range(2)]
    toks[1].pad_token = "!"
    sds = [Wt.synthetic_clip_state_dict(128, 3, 512, vocab=len(toks[0]), seed=5, dtype=BF),
           Wt.synthetic_clip_state_dict(128, 4, 512, vocab=len(toks[0]), proj=96, seed=6, dtype=BF)]
    meta = [(2, "quick_gelu", 2), (2, "gelu", 2)]
    encs = [T.ClipTextEncoder(sd, h, a, e) for sd, (h, a, e) in zip(sds, meta)]
    long_p = " ".join(["photo of a cat and a dog running , mountain background"] * 9)          # 99 tokens
    prompts = [long_p, "a teddy bear"]
    chunks = T.chunk_prompt(toks, long_p)
    assert len(chunks) == 2
    emb, pooled = T.encode_prompts(encs, toks, prompts, long=True)
    assert emb.shape == (2, 154, 256) and emb.dtype == BF and pooled.shape == (2, 96)
    four = [chunks[0], chunks[1], "a teddy bear", ""]
    e4, p4 = T.encode_prompts(encs, toks, four)                              # short path: four prompts of 77
    assert e4.shape == (4, 77, 256)
    assert torch.equal(emb, torch.cat([torch.cat([e4[0], e4[1]])[None], torch.cat([e4[2], e4[3]])[None]]))
    assert torch.equal(pooled, p4[[0, 2]])
    # a run count from elsewhere pads with empty chunks and leaves the first chunks' bits alone
    e3, p3 = T.encode_prompts(encs, toks, ["a teddy bear"], long=True, chunks=3)
    assert e3.shape == (1, 231, 256) and torch.isfinite(e3.float()).all()
    # one chunk, long: the short path's ids, so its bits
    e1, p1 = T.encode_prompts(encs, toks, ["a teddy bear"], long=True)
    e0, p0 = T.encode_prompts(encs, toks, ["a teddy bear"])
    assert torch.equal(e1, e0) and torch.equal(p1, p0)
    # the oracle per chunk
    ids = [t(four) for t in toks]
    want_e, want_p = CO.encode_prompt([({k: v.float() for k, v in sd.items()}, h, a, e) for sd, (h, a, e) in zip(sds, meta)], ids)
    for r in range(4):
        got = emb[r // 2, 77 * (r % 2):77 * (r % 2) + 77]
        print(f"chunk row {r}: hidden rel L2 {_rel(got, want_e[r]):.3g}")
        assert _rel(got, want_e[r]) < 2e-2
    assert _rel(pooled, want_p[[0, 2]]) < 3e-2


# ------------------------------------------------------------------------------------------------ 8. plans
def _tiny_case(Lk, B=2, seed=1):
    from oracle import unet_oracle as UO
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    W = U.UNetWeights(cfg, sd, "cuda")
    orc = UO.UNetOracle(UO.TINY, sd)
    g = torch.Generator().manual_seed(seed)
    ehs = torch.randn(B, Lk, cfg.cross_dim, generator=g).to(BF).float()
    pooled = torch.randn(B, cfg.pooled_dim, generator=g)
    tid = torch.tensor([[128, 128, 0, 0, 128, 128]] * B, dtype=torch.float32)
    return cfg, W, orc, ehs, pooled, tid


def _names(p):
    return [getattr(fn, "__name__", "") for fn, _a in p.ops]


@pytest.mark.parametrize("Lk,fp8", [(154, False), (231, False), (154, True)])
def test_plain_plan_over_chunked_keys_matches_the_oracle(Lk, fp8, monkeypatch):
    """the plain plan's existing bound (2e-2 rel L2; tests/test_unet_gpu.py) in bf16; the fp8 plan against the tiny fp8 plan's (3e-2)"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import unet as U
    cfg, W, orc, ehs, pooled, tid = _tiny_case(Lk)
    kv = U.KVCache(W, ehs, [0, 0])
    assert kv.Lk == Lk and kv.ld == (Lk + 7) // 8 * 8
    plan = U.UNetPlan(W, 2, 16, 16, kv, pooled, tid, fp8=fp8)
    x = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(4)).repeat(2, 1, 1, 1)
    eps = plan(x.cuda(), 601).float().cpu()
    ref = orc.forward(x, 601, ehs, pooled, tid).float()
    r = _rel(eps, ref)
    print(f"plain plan, {Lk} keys, fp8={fp8}: rel L2 {r:.3g}")
    assert torch.isfinite(eps).all() and r <= (3e-2 if fp8 else 2e-2), r
    assert "tmix_gemm_q_cross_attn" not in _names(plan) and not plan._qattn
    assert torch.equal(plan(x.cuda(), 601).float().cpu(), eps)
    # the keys of the second chunk matter: without them the result moves
    short = U.UNetPlan(W, 2, 16, 16, U.KVCache(W, ehs[:, :77].contiguous(), [0, 0]), pooled, tid, fp8=fp8)
    assert not torch.equal(short(x.cuda(), 601).float().cpu(), eps)


def test_a_77_key_plan_records_the_launches_it_always_did(monkeypatch):
    """77 keys: the one-launch attn2 gate stays open, a probe of <= 8 positions records tmix_xattn_token_maps; only past 80 keys or
    8 positions does a plan record the long entry point, and nothing else about it changes"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import unet as U
    cfg, W, orc, ehs, pooled, tid = _tiny_case(154)
    e77 = ehs[:, :77].contiguous()
    mk = lambda e, **kw: U.UNetPlan(W, 2, 16, 16, U.KVCache(W, e, [0, 0]), pooled, tid, **kw)
    p77, p154 = mk(e77), mk(ehs)
    assert p77._qattn and p77.kv.ld == 80
    assert _names(p77) == _names(p154)                  # (the tiny grids are below the one-launch form's size gate: the pair at both key counts)
    assert not any("xattn" in n for n in _names(p77))
    spec8 = U.TokenMapSpec((1, 4, 7, 31, 32, 63, 64, 76))
    probe8 = mk(e77, token_maps=spec8)
    assert _names(probe8).count("tmix_xattn_token_maps") == 17 and "tmix_xattn_token_maps_long" not in _names(probe8)
    probe9 = mk(e77, token_maps=U.TokenMapSpec((1, 4, 7, 31, 32, 63, 64, 76, 9)))
    assert _names(probe9).count("tmix_xattn_token_maps_long") == 17 and "tmix_xattn_token_maps" not in _names(probe9)
    strip = lambda p: [n for n in _names(p) if "xattn" not in n]
    assert strip(probe8) == strip(probe9) == _names(p77)
    x = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(4)).repeat(2, 1, 1, 1).cuda()
    e8, e9 = probe8(x, 601).clone(), probe9(x, 601).clone()
    assert torch.equal(e8, e9) and torch.equal(e8, p77(x, 601))              # the maps are a side output
    for lvl in probe8.token_maps:
        a, b = probe8.token_maps[lvl], probe9.token_maps[lvl][:, :8]
        assert (a - b).abs().max().item() <= 1e-4 * 4 * 17                   # 1e-4 * H per launch, H <= 4, at most 17 launches summed


# ------------------------------------------------------------------------------------------------ 9. probe plan
def _recording_oracle(base):
    """UNetOracle whose attn2 also records the conditional row's probabilities at the tokens, summed over heads and modules per level
    (restated from tests/test_attn_masks_gpu.py)"""
    from oracle import unet_oracle as UO

    class Recording(UO.UNetOracle):
        tokens, row, maps = (), 1, None

        def _attn(self, x, ehs, name, routed):
            out = super()._attn(x, ehs, name, routed)
            if ehs is not None:
                H = x.shape[-1] // self.cfg.head_dim
                q = self._lin(x[self.row:self.row + 1], name + ".to_q")[0]
                k = self._lin(ehs[self.row:self.row + 1], name + ".to_k")[0]
                qh = q.view(-1, H, 64).transpose(0, 1)
                kh = k.view(-1, H, 64).transpose(0, 1)
                p = torch.softmax(qh @ kh.transpose(1, 2) * self.cfg.head_dim ** -0.5, dim=-1)
                m = p[:, :, list(self.tokens)].sum(0).transpose(0, 1).float().cpu()
                S = x.shape[1]
                self.maps[S] = self.maps.get(S, 0) + m
            return out

    rec = Recording.__new__(Recording)
    rec.__dict__.update(base.__dict__)
    rec.maps = {}
    return rec


def test_probe_plan_with_nine_positions_across_two_chunks_matches_the_oracle(monkeypatch):
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import unet as U
    cfg, W, orc, ehs, pooled, tid = _tiny_case(154)
    tokens = [4, 7, 9, 76, 77 + 5, 100, 127, 128, 153]
    probe = U.UNetPlan(W, 2, 16, 16, U.KVCache(W, ehs, [0, 0]), pooled, tid, token_maps=U.TokenMapSpec(tuple(tokens), row0=1, row_step=2, n_rows=1))
    plain = U.UNetPlan(W, 2, 16, 16, U.KVCache(W, ehs, [0, 0]), pooled, tid)
    assert [n for n in _names(probe) if n != "tmix_xattn_token_maps_long"] == _names(plain)
    assert _names(probe).count("tmix_xattn_token_maps_long") == len(U.attention_blocks(cfg)) == 17
    x = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(4)).repeat(2, 1, 1, 1)
    eps = probe(x.cuda(), 601).float().cpu()
    assert torch.equal(eps, plain(x.cuda(), 601).float().cpu())
    rec = _recording_oracle(orc)
    rec.tokens = tokens
    ref = rec.forward(x, 601, ehs, pooled, tid).float()
    assert _rel(eps, ref) <= 2e-2
    for lvl, m in probe.token_maps.items():
        S = (16 >> lvl) * (16 >> lvl)
        r = _rel(m[0], rec.maps[S])
        print(f"probe over 154 keys, level {lvl}: maps rel L2 {r:.3g}")
        assert m.shape == (1, 9, S) and r <= 2e-2, (lvl, r)                 # the bound of tests/test_attn_masks_gpu.py's probe test


# ------------------------------------------------------------------------------------------------ every call kind of the sampler
def _tiny_sampler_inputs(kind, Lk, K=3):
    from tweediemix_amd import unet as U, weights as Wt
    cfg = U.TINY
    sd = Wt.synthetic_state_dict(cfg, seed=1234, nontrivial=True)
    con = Wt.synthetic_concepts(cfg, kind, K)
    g = torch.Generator().manual_seed(0)
    te = (torch.randn(K + 2, Lk, cfg.cross_dim, generator=g).to(BF).float(), torch.randn(K + 2, cfg.pooled_dim, generator=g))
    ts = (torch.randn(K, Lk, cfg.cross_dim, generator=g).to(BF).float(), torch.randn(K, cfg.pooled_dim, generator=g))
    return U.UNetWeights(cfg, sd, "cuda", (kind, con)), te, ts


def _no_provider(x0):
    raise AssertionError("the mask provider must not be called with attention_masks")


@pytest.mark.parametrize("kind,fp8,Lk", [("custom", False, 154), ("lora", False, 231), ("lora", True, 154)])
def test_sampler_runs_every_call_kind_over_chunked_keys(kind, fp8, Lk, monkeypatch):
    """fusion, fusion_base (LoRA outside its window), start, plain and probe plans over 154 / 231 keys in one trajectory, graphs on,
    nine positions probed; a second run is bit-identical"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    W, te, ts = _tiny_sampler_inputs(kind, Lk)
    cfg = S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=2,
                        resolution_h=h * 8, resolution_w=w * 8)
    am = dict(tokens=[[4, 5, 6, 80, 81], [7, 9, 100, Lk - 1]])
    xT = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(7))
    lats = []
    for _ in range(2):
        tw = S.Tweediemix(cfg, W, te, ts, _no_provider, concept_num=K, lora=(kind == "lora"), use_graphs=True, fp8=fp8, attention_masks=am)
        lats.append(tw.run_fusion(xT.clone()).cpu())
    assert torch.isfinite(lats[0]).all() and torch.equal(lats[0], lats[1])
    kinds = {c[0] for c in tw.unet_calls}
    assert {"fusion", "start", "plain", "probe"} <= kinds and (kind != "lora" or "fusion_base" in kinds), kinds
    assert all(p.kv.Lk == Lk for p in tw.plans.values())
    assert tw.attention_maps[0][1].shape == (9, 8, 8)


def test_co_batched_seeds_over_154_keys_match_their_single_runs(monkeypatch):
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    from tweediemix_amd import sampler as S
    K, h, w = 3, 16, 16
    W, te, ts = _tiny_sampler_inputs("custom", 154)
    cfg = S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, t_stop=0.8, resampling_steps=1, jumping_steps=2,
                        resolution_h=h * 8, resolution_w=w * 8)
    am = dict(tokens=[[4, 80], [7, 153]])
    xT = torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(8))
    singles = []
    for i in range(2):
        tw = S.Tweediemix(cfg, W, te, ts, _no_provider, concept_num=K, attention_masks=am)
        singles.append((tw.run_fusion(xT[i:i + 1].clone()).cpu(), tw.masks.clone().cpu()))
    tw2 = S.Tweediemix(cfg, W, te, ts, _no_provider, concept_num=K, attention_masks=am, n_seeds=2, use_graphs=True)
    both = tw2.run_fusion(xT.clone()).cpu()
    assert tw2.plan("probe").B == 4 and tw2.plan("probe").kv.Lk == 154
    for i in range(2):
        assert torch.equal(tw2.masks[i].cpu(), singles[i][1]), i
        assert (both[i:i + 1] - singles[i][0]).abs().max().item() <= 1e-3, i      # tests/test_sampler_gpu.py's bound for co-batched seeds


# ------------------------------------------------------------------------------------------------ 10. end to end
def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_long_gpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def test_cli_long_prompts_end_to_end(tmp_path, monkeypatch):
    """--synthetic --tiny: two chunks with attention masks from nine positions run to a finite latent; one chunk with the flag is the
    run without it, bit for bit"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    fs = _cli()
    common = ["--synthetic", "--tiny", "--seed", "5", "--concepts", "cat+dog+mountain", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p",
              "--guidance_scale", "0.8", "--n_timesteps", "10", "--t_cond", "0.2", "--resampling_steps", "1", "--jumping_steps", "2",
              "--resolution_h", "128", "--resolution_w", "128", "--mask_source", "attention"]
    out = lambda n: ["--output_path", str(tmp_path / n), "--output_path_all", str(tmp_path / n / "all")]
    nine = "4,5,6,80,81+7,9,100,153"
    lat2 = fs.main(common + out("two") + ["--long_prompts", "--synthetic_chunks", "2", "--mask_token_ids", nine, "--save_attention_maps"])
    assert lat2.shape == (1, 4, 16, 16) and torch.isfinite(lat2).all()
    import numpy as np
    m = np.load(tmp_path / "two" / "attention_maps_5_level1.npy")
    assert m.shape == (9, 8, 8) and np.isfinite(m).all() and m.max() > 0
    with pytest.raises(SystemExit, match="153"):
        fs.main(common + out("bad") + ["--long_prompts", "--synthetic_chunks", "2", "--mask_token_ids", "4+154"])
    base = fs.main(common + out("base") + ["--mask_token_ids", "4+7,9"])
    one = fs.main(common + out("one") + ["--long_prompts", "--synthetic_chunks", "1", "--mask_token_ids", "4+7,9"])
    assert torch.equal(one, base)
    assert not torch.equal(lat2, base)


def _checkpoint(tmp_path, golden_dir):
    """a synthetic diffusers-layout SDXL checkpoint folder without a VAE (text towers, tokenizers, tiny UNet, three concepts), as in
    tests/test_attn_masks_gpu.py"""
    import json
    import shutil
    import numpy as np
    from safetensors.torch import save_file
    from tweediemix_amd import unet as U, weights as Wt
    sdp = tmp_path / "sdxl"
    z = np.load(os.path.join(golden_dir, "clip_text.npz"))
    g = torch.Generator().manual_seed(11)
    for folder, name, act in (("text_encoder", "l", "quick_gelu"), ("text_encoder_2", "g", "gelu")):
        sd = {k[len(name) + 4:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(name + ".sd.")}
        key = [k for k in sd if k.endswith("token_embedding.weight")][0]
        sd[key] = torch.cat([sd[key], torch.randn(620 - 64, 128, generator=g) * 0.05])      # the tokenizer fixture has 615 ids
        (sdp / folder).mkdir(parents=True)
        save_file({k: v.contiguous() for k, v in sd.items()}, str(sdp / folder / "model.safetensors"))
        json.dump({"hidden_act": act, "num_attention_heads": 2, "eos_token_id": 2, "layer_norm_eps": 1e-5},
                  open(sdp / folder / "config.json", "w"))
    for folder, pad in (("tokenizer", "<|endoftext|>"), ("tokenizer_2", "!")):
        shutil.copytree(os.path.join(golden_dir, "clip_tok"), sdp / folder)
        json.dump({"pad_token": pad}, open(sdp / folder / "special_tokens_map.json", "w"))
    ucfg = {"block_out_channels": [64, 128, 256], "layers_per_block": 2, "transformer_layers_per_block": [1, 1, 2],
            "down_block_types": ["DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"], "attention_head_dim": [1, 2, 4],
            "cross_attention_dim": 256, "addition_time_embed_dim": 32, "projection_class_embeddings_input_dim": 96 + 6 * 32}
    cfg = U.UNetConfig.from_diffusers(ucfg)
    (sdp / "unet").mkdir()
    json.dump(ucfg, open(sdp / "unet" / "config.json", "w"))
    save_file({k: v.cpu().contiguous() for k, v in Wt.synthetic_state_dict(cfg, seed=3, device="cpu", dtype=torch.float16).items()},
              str(sdp / "unet" / "diffusion_pytorch_model.fp16.safetensors"))
    ckpts = []
    for i, con in enumerate(Wt.synthetic_concepts(cfg, "custom", 3, device="cpu")):
        fp = tmp_path / f"delta{i}.bin"
        torch.save({"unet": con, "modifier_token": {f"<new{i + 1}>": torch.randn(128, generator=g) * 0.1},
                    "modifier_token_2": {f"<new{i + 1}>": torch.randn(128, generator=g) * 0.1}}, fp)
        ckpts.append(str(fp))
    return sdp, ckpts


def test_cli_long_scene_prompt_through_the_text_towers(tmp_path, golden_dir, monkeypatch):
    """a checkpoint folder and a scene prompt of 88 tokens whose --seg_concepts phrases lie in the second chunk: the towers encode two
    chunks per row, the phrases are found at 77 + offset, the masks and maps come out; without the flag the same phrases are cut off"""
    need_gpu()
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    import numpy as np
    from tweediemix_amd import text as T
    sdp, ckpts = _checkpoint(tmp_path, golden_dir)
    fs = _cli()
    scene = " ".join(["mountain background"] * 40) + " photo of a cat and a dog running"
    toks = [T.ClipBPETokenizer.from_pretrained(str(sdp / "tokenizer")), T.ClipBPETokenizer.from_pretrained(str(sdp / "tokenizer_2"))]
    assert len(T.chunk_prompt(toks, scene)) == 2
    assert T.token_positions_long(toks, scene, "a cat") == [77 + 9] and T.token_positions_long(toks, scene, "a dog") == [77 + 12]
    out = tmp_path / "out"
    argv = ["--sd_path", str(sdp), "--personal_checkpoint", "+".join(ckpts), "--seed", "9", "--mask_source", "attention",
            "--save_attention_maps", "--prompt", "photo of a cat running+photo of a dog running+mountain background",
            "--prompt_orig", scene, "--concepts", "cat+dog+mountain", "--modifier_token", "<new1>+<new2>+<new3>",
            "--seg_concepts", "a cat+a dog", "--guidance_scale", "0.8", "--n_timesteps", "10", "--t_cond", "0.2",
            "--resampling_steps", "1", "--jumping_steps", "2", "--resolution_h", "128", "--resolution_w", "128",
            "--output_path", str(out), "--output_path_all", str(out / "all")]
    lat = fs.main(argv + ["--long_prompts"])
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all()
    assert len(scene) > 255 and len(fs.output_stem(scene)) <= 200                  # the scene prompt itself is no file name
    assert torch.equal(torch.load(out / "all" / f"{fs.output_stem(scene)}_9.latent.pt"), lat.cpu())
    for lvl, side in ((1, 8), (2, 4)):
        m = np.load(out / f"attention_maps_9_level{lvl}.npy")
        assert m.shape == (2, side, side) and np.isfinite(m).all() and m.max() > 0
    with pytest.raises(SystemExit, match="does not occur"):       # today's 77-token cut drops the phrases: the lookup says so
        fs.main(argv)
