"""CPU: the image UNet (UNetPlan) and the video UNet (I2VPlan) record through the same op emitters, the methods of unet.BlockPlan over
plan.LaunchPlan.  Every attribute those methods read through `self.` must be assigned by the two base constructors (or by the method
itself before it reads it) -- whatever a derived plan happens to set does not count.  (Round 3 broke the weaker form of this once: a new
`self.lowrank` read in _t2d made the video plan -- and with it the default bench line -- fail with AttributeError.)  The emitters read
that state as plain `self.X`: a getattr(self, "X", default) would hand a plan a default nobody chose and hide the read from this check.
Both derived constructors must reach the base constructors through super().  Checked statically on the sources."""
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


def _self_writes(node):
    out = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name) and n.value.id == "self":
            out.add(n.attr)
    return out


def _getattr_self(fn):
    """names read as getattr(self, "X", ...) inside fn"""
    return {n.args[1].value for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr"
            and len(n.args) >= 2 and isinstance(n.args[0], ast.Name) and n.args[0].id == "self" and isinstance(n.args[1], ast.Constant)}


def _methods(cls):
    return {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}


def _calls_super_init(fn):
    """does fn contain super().__init__(...)?"""
    return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "__init__" and isinstance(n.func.value, ast.Call)
               and isinstance(n.func.value.func, ast.Name) and n.func.value.func.id == "super" and not n.func.value.args for n in ast.walk(fn))


def test_video_plan_sets_every_attribute_the_shared_emitters_read():
    base = _cls("tweediemix_amd/plan.py", "LaunchPlan")
    block = _cls("tweediemix_amd/unet.py", "BlockPlan")
    unet = _cls("tweediemix_amd/unet.py", "UNetPlan")
    i2v = _cls("tweediemix_amd/i2vgen.py", "I2VPlan")
    assert [b.id for b in block.bases] == ["LaunchPlan"] and [b.id for b in unet.bases] == ["BlockPlan"] and [b.id for b in i2v.bases] == ["BlockPlan"]
    mb, mk = _methods(base), _methods(block)
    shared = [m for name, m in list(mb.items()) + list(mk.items()) if name != "__init__"]
    assert {"_gn", "_conv", "_gemm", "_t2d", "_proj", "_resnet", "_launch", "_emit", "run", "issued_meta"} <= {m.name for m in shared}, "the emitters both networks record through"
    # the constructor chain: each derived plan -> BlockPlan -> LaunchPlan, through super()
    for c in (unet, i2v, block):
        assert _calls_super_init(_methods(c)["__init__"]), f"{c.name}.__init__ must call super().__init__"
    # what a shared method can find on self: the base classes' methods and class attributes, and what the two base constructors assign
    have = _self_writes(mb["__init__"]) | _self_writes(mk["__init__"]) | set(mb) | set(mk)
    have |= {t.id for n in base.body + block.body if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
    missing = {}
    for m in shared:
        need = _self_reads(m) - have - _self_writes(m)          # (an attribute the method itself assigns before reading it: a cache)
        if need:
            missing[m.name] = sorted(need)
    assert not missing, f"shared emitters read attributes the base constructors never set: {missing}"
    own = [m for c in (unet, i2v) for m in _methods(c).values()]
    hidden = {m.name: sorted(_getattr_self(m)) for m in shared + own + [mb["__init__"], mk["__init__"]] if _getattr_self(m)}
    assert not hidden, f"plan state read through getattr(self, name, default) instead of self.name: {hidden}"
