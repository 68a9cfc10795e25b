"""CPU: the video plan (I2VPlan) reuses the image UNet's op emitters.  Both plans' constructors set the emitters' common state through
UNetPlan._init_emit_state and each sets the rest itself, so every attribute those emitters read through `self.` must be set by I2VPlan
or by _init_emit_state.  (Round 3 broke exactly that once: a new `self.lowrank` read in UNetPlan._t2d made the video plan -- and with
it the default bench line -- fail with AttributeError.)  The emitters read that state as plain `self.X`: a getattr(self, "X", default)
would hand the video plan a default nobody chose and hide the read from this check.  Checked statically on the sources."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cls(path, name):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == name)


def _self_reads(fn):
    """attribute names read as self.X inside fn (not assignment targets)"""
    stores = {id(n) for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store)}
    return {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and id(n) not in stores
            and isinstance(n.value, ast.Name) and n.value.id == "self"}


def _self_writes(cls):
    out = set()
    for n in ast.walk(cls):
        if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name) and n.value.id == "self":
            out.add(n.attr)
    return out


def _getattr_self(fn):
    """names read as getattr(self, "X", ...) inside fn"""
    return {n.args[1].value for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr"
            and len(n.args) >= 2 and isinstance(n.args[0], ast.Name) and n.args[0].id == "self" and isinstance(n.args[1], ast.Constant)}


def test_video_plan_sets_every_attribute_the_shared_emitters_read():
    unet = _cls("tweediemix_amd/unet.py", "UNetPlan")
    i2v = _cls("tweediemix_amd/i2vgen.py", "I2VPlan")
    methods = {n.name: n for n in unet.body if isinstance(n, ast.FunctionDef)}
    own = {n.name: n for n in i2v.body if isinstance(n, ast.FunctionDef)}
    shared = [m for name, m in methods.items() if name not in own and name not in ("__init__", "_build")]
    assert {"_gn", "_conv", "_gemm", "_t2d", "_proj", "_resnet"} <= {m.name for m in shared}, "the emitters the video plan borrows"
    calls = lambda fn: {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
                        and isinstance(n.func.value, ast.Name) and n.func.value.id == "self"}
    assert "_init_emit_state" in calls(methods["__init__"]) and "_init_emit_state" in calls(own["__init__"])
    # what the borrowed emitters can call on self: UNetPlan's methods / class attributes, I2VPlan's own, and everything I2VPlan or
    # _init_emit_state assigns
    have = _self_writes(i2v) | _self_writes(methods["_init_emit_state"]) | set(methods) | set(own)
    have |= {t.id for n in unet.body + i2v.body if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
    # attributes a borrowed emitter itself creates before reading them (caches)
    for m in shared:
        have |= {n.attr for n in ast.walk(m) if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name) and n.value.id == "self"}
    missing = {}
    for m in shared:
        need = _self_reads(m) - have
        if need:
            missing[m.name] = sorted(need)
    assert not missing, f"UNetPlan emitters read attributes I2VPlan never sets: {missing}"
    hidden = {m.name: sorted(_getattr_self(m)) for m in shared + list(own.values()) if _getattr_self(m)}
    assert not hidden, f"plan state read through getattr(self, name, default) instead of self.name: {hidden}"
