"""CPU: the launch recorder (tweediemix_amd/plan.py) on its own -- CPU tensors, and stub entry points that carry the library's names,
record their calls and return a chosen code.  What every plan relies on: where the weight hints go and what they name, that the
bookkeeping bench.py and the tuner read follows from what was recorded, that a stamped launch recorded as a plain op fails when the
plan is frozen, how run() ends at a failing launch, and how the arena hands buffers on."""
import pytest
import torch

from tweediemix_amd import lib as L
from tweediemix_amd import plan as P


class StubLib:
    """getattr(lib, name) -> a callable named `name` that appends (name, args) to .calls and returns .rc.get(name, 0)"""

    def __init__(self):
        self.calls, self.rc, self._fns = [], {}, {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self._fns:
            def fn(*args, _n=name):
                self.calls.append((_n, args))
                return self.rc.get(_n, 0)
            fn.__name__ = name
            self._fns[name] = fn
        return self._fns[name]


def recorder(hints=(0, 0)):
    return P.LaunchPlan(torch.device("cpu"), hints, lib=StubLib())


def weight(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8)


def names(plan):
    return [fn.__name__ for fn, _a in plan.ops]


def test_every_hinted_launch_is_preceded_by_a_hint_that_names_the_next_hinted_weight():
    cap, over = 4096, 8192
    p = recorder((cap, over))
    ws = [weight(1000), weight(over), weight(over + 1), weight(100000)]
    d = [object() for _ in ws]
    p._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=d[0], weight=ws[0], tunable="gemm")
    p._launch("tmix_groupnorm_nhwc", (2,), 0, key=("norm", 1, 2, 3))             # not hinted: no slot, and it does not break the chain
    p._launch("tmix_conv3x3_nhwc", (3,), 20, desc=d[1], weight=ws[1], tunable="conv")
    p._emit(p.lib.tmix_concat_channels, 4)
    p._launch("tmix_gemm_fp8", (5,), 30, gemm_flops=30, desc=d[2], weight=ws[2])
    p._launch("tmix_conv3x3_nhwc", (6,), 40, desc=d[3], weight=None, tunable="conv")     # weight=None: a launch that is never hinted
    p._launch("tmix_gemm_q_cross_attn", (7,), 50, gemm_flops=45, desc=d[3], weight=ws[3])
    p._freeze()
    assert names(p) == ["tmix_gemm_prefetch_next", "tmix_gemm_bf16", "tmix_groupnorm_nhwc", "tmix_gemm_prefetch_next", "tmix_conv3x3_nhwc",
                        "tmix_concat_channels", "tmix_gemm_prefetch_next", "tmix_gemm_fp8", "tmix_conv3x3_nhwc", "tmix_gemm_prefetch_next",
                        "tmix_gemm_q_cross_attn"]
    slots = [a for fn, a in p.ops if fn.__name__ == "tmix_gemm_prefetch_next"]
    # the slot in front of hinted launch i names the weight of hinted launch i + 1; the cap bites only above `over`
    assert slots == [(ws[1].data_ptr(), over), (ws[2].data_ptr(), cap), (ws[3].data_ptr(), cap), (None, 0)]
    assert [s[1] for s in slots[:3]] == [P.hint_bytes(w.numel(), cap, over) for w in ws[1:]]
    assert all(any(k is w for k in p.keep) for w in ws)                             # a hinted weight outlives the plan's hints


def test_no_hint_op_is_recorded_with_hints_switched_off_or_without_weights(monkeypatch):
    monkeypatch.setenv("TMIX_NO_PREFETCH", "1")
    p = recorder()
    p._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=object(), weight=weight(64), tunable="gemm")
    p._launch("tmix_conv3x3_nhwc", (2,), 10, desc=object(), weight=weight(64), tunable="conv")
    assert names(p) == ["tmix_gemm_bf16", "tmix_conv3x3_nhwc"] and [i for i, _k, _d in p._tunable] == [0, 1]
    monkeypatch.delenv("TMIX_NO_PREFETCH")                                          # (read when the plan is constructed)
    q = recorder()
    q._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=object())         # the VAE's form: no weight, no hint
    assert names(q) == ["tmix_gemm_bf16"]
    r = recorder()
    r._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=object(), weight=weight(64))
    assert names(r) == ["tmix_gemm_prefetch_next", "tmix_gemm_bf16"]


def test_bookkeeping_follows_from_what_was_recorded():
    p = recorder()
    dg, dq, d8, dc, dc8 = (object() for _ in range(5))
    attn_args = (11, 12, 13)
    p._emit(p.lib.tmix_conv_in, 0)
    p._launch("tmix_gemm_bf16", (1,), 100, gemm_flops=100, desc=dg, weight=weight(8), tunable="gemm")
    p._launch("tmix_gemm_q_cross_attn", (2,), 130, gemm_flops=90, desc=dq, weight=weight(8))
    p._launch("tmix_gemm_fp8", (3,), 200, gemm_flops=200, desc=d8, weight=weight(8))
    p._launch("tmix_conv3x3_nhwc", (4,), 300, desc=dc, weight=weight(8), tunable="conv")
    p._launch("tmix_conv3x3_nhwc_fp8", (5,), 400, desc=dc8, weight=weight(8))
    for name in ("tmix_groupnorm_nhwc", "tmix_groupnorm_nhwc_pre", "tmix_groupnorm_nhwc_pre_f8"):
        p._launch(name, (6,), 0, key=("norm", name))
    p._launch("tmix_attn_fwd_ws", attn_args, 500, key=("attn", 1))
    p._launch("tmix_attn_fwd_f8_ws", attn_args, 600, key=("attn", 2))
    p._emit(p.lib.tmix_conv_out, 9)
    p._freeze()
    meta = p.issued_meta()
    # the class comes from the entry point
    assert [m[0] for m in meta] == ["gemm", "gemm", "gemm_fp8", "conv", "conv_fp8", "norm", "norm", "norm", "attn", "attn"]
    assert [m[1] for m in meta] == [100, 130, 200, 300, 400, 0, 0, 0, 500, 600]
    assert [m[2] for m in meta[:5]] == [dg, dq, d8, dc, dc8] and meta[8][2] == ("attn", 1)
    # issue order: op_meta's keys are the positions of exactly the stamped ops
    stamped = [i for i, (fn, _a) in enumerate(p.ops) if fn.__name__ in P.STAMPED]
    assert sorted(p.op_meta) == stamped and meta == [p.op_meta[i] for i in stamped]
    assert p.flops == sum(m[1] for m in meta) and p.gemm_flops == 100 + 90 + 200
    assert p.launches == {"gemm": [(dg, 100), (dq, 90), (d8, 200)], "conv": [(dc, 300), (dc8, 400)], "attn": [(attn_args, 500), (attn_args, 600)]}
    assert [(p.ops[i][0].__name__, k, d) for i, k, d in p._tunable] == [("tmix_gemm_bf16", "gemm", dg), ("tmix_conv3x3_nhwc", "conv", dc)]
    assert all(any(k is d for k in p.keep) for d in (dg, dq, d8, dc, dc8))
    assert set(P.STAMPED.values()) == {"gemm", "gemm_fp8", "conv", "conv_fp8", "norm", "attn"} and set(P.STAMPED) <= set(L.SIGNATURES)


def test_freezing_makes_tuples_and_refuses_a_stamped_launch_recorded_as_a_plain_op():
    p = recorder()
    p._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=object(), weight=weight(8))
    assert isinstance(p.ops[0][1], list)                                            # the open hint slot
    p._freeze()
    assert all(isinstance(a, tuple) for _fn, a in p.ops) and p.ops[0][1] == (None, 0)
    for name in P.STAMPED:
        q = recorder()
        q._emit(getattr(q.lib, name), 1)
        with pytest.raises(AssertionError, match=name):
            q._freeze()
    q = recorder()
    q._emit(q.lib.tmix_softmax_rows, 1)
    q.op_meta[0] = ("gemm", 0, None)                                                # an entry for an op the library does not stamp
    with pytest.raises(AssertionError, match="tmix_softmax_rows"):
        q._freeze()
    with pytest.raises(KeyError):
        recorder()._launch("tmix_softmax_rows", (1,), 0)                            # _launch takes stamped entry points only
    # a library whose functions are wrapped (a test that logs every call): the class comes from the name _launch is given, not from the callable
    class Wrapped:
        def __getattr__(self, name):
            return lambda *a: 0
    w = P.LaunchPlan(torch.device("cpu"), lib=Wrapped())
    w._launch("tmix_gemm_bf16", (1,), 10, gemm_flops=10, desc=object(), weight=weight(8))
    w._emit(w.lib.tmix_conv_in, 1)
    w._freeze()
    assert [m[0] for m in w.issued_meta()] == ["gemm"] and sorted(w.op_meta) == [1]


def test_run_passes_the_stream_last_and_stops_at_the_first_failing_launch():
    p = recorder()
    p._emit(p.lib.tmix_conv_in, 1, 2)
    p._launch("tmix_gemm_bf16", (3,), 10, gemm_flops=10, desc=object(), weight=weight(8))
    p._launch("tmix_groupnorm_nhwc", (4,), 0, key=("norm",))
    p._emit(p.lib.tmix_conv_out, 5)
    p._freeze()
    p.run(stream=77)
    assert p.lib.calls == [("tmix_conv_in", (1, 2, 77)), ("tmix_gemm_prefetch_next", (None, 0, 77)), ("tmix_gemm_bf16", (3, 77)),
                           ("tmix_groupnorm_nhwc", (4, 77)), ("tmix_conv_out", (5, 77))]
    del p.lib.calls[:]
    p.lib.rc["tmix_gemm_bf16"] = L.ESHAPE
    with pytest.raises(L.TmixError, match="tmix_gemm_bf16"):
        p.run(stream=77)
    assert [n for n, _a in p.lib.calls] == ["tmix_conv_in", "tmix_gemm_prefetch_next", "tmix_gemm_bf16"]


def test_arena_hands_a_released_buffer_to_the_next_request_of_the_same_rounded_size():
    A = P.Arena(torch.device("cpu"))
    a = A.get(3, 50)                                # 300 bytes of bf16 -> one 512-byte buffer
    b = A.get(2, 2, dtype=torch.float32)            # 16 bytes -> 256
    assert A.total == 512 + 256 and a.data_ptr() != b.data_ptr()
    A.put(a)
    c = A.get(7, dtype=torch.float32)               # 28 bytes -> 256: another size class, a new buffer
    assert c.data_ptr() not in (a.data_ptr(), b.data_ptr()) and A.total == 512 + 512
    d = A.get(200, dtype=torch.bfloat16)            # 400 bytes -> 512: the buffer a lived in
    assert d.data_ptr() == a.data_ptr() and d.shape == (200,) and d.dtype == torch.bfloat16 and A.total == 1024
    A.put(b, c)
    assert A.get(64, dtype=torch.uint8).data_ptr() == c.data_ptr()                  # last released, first reused


def test_arena_releases_the_column_partials_that_travel_with_a_tensor():
    A = P.Arena(torch.device("cpu"))
    x = A.get(4, 64, 8)
    cs = A.get(8, 2, 8, dtype=torch.float32)
    x._cs = ((cs, 8),)
    A.put(x)
    assert x._cs is None
    assert A.get(8, 2, 8, dtype=torch.float32).data_ptr() == cs.data_ptr() and A.get(4, 64, 8).data_ptr() == x.data_ptr()
    assert len(A.bufs) == 2
