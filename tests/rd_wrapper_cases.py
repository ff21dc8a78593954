"""The case tables of the Python wrappers of the device-resident calls (rd.QueryRays .. rd.TraceAreaPathsTorch): what each wrapper
asks of the library, what it returns, what it refuses and in which words, and the public surface of rd.py.  Shared by
tests/golden/make_rd_wrappers.py (the recorder), tests/test_rd_wrappers_cpu.py and the child of tests/test_gpu_rd_wrappers.py.

Nothing here needs librdx.so or a scene: `stand_in` puts a Recorder in the place of `_lib.lib()`.  A case is (id, thunk); `outcome`
runs the thunk under the stand-in and returns plain data -- the library calls in order, and what came back or the refusal's text --
which is what tests/golden/rd_wrappers.json holds, recorded at the commit before the wrappers were put on one argument layer.
"""
import contextlib
import ctypes as C
import hashlib
import inspect
import itertools
import json

import numpy as np

BUFFER_ROUTE = ("QueryRays", "ResolveHits", "ShadeHits", "ResolveMaterials", "LightHits", "ScatterHits", "GenerateRays", "Accumulate", "TracePaths",
                "TraceLightPaths", "PunctualLightHits", "TracePunctualPaths", "AreaLightHits", "TraceAreaPaths")
TORCH_ROUTE = tuple(name + "Torch" for name in BUFFER_ROUTE)
OUT_WORD = 7        # what the stand-in writes into every byref output word (live, invalid)


# ---- the stand-in for _lib.lib() ------------------------------------------------------------------------------------------------------
class Recorder:
    """every attribute is a library function: it records its name and arguments (a byref struct as its fields, a byref output word
    as "out", after writing OUT_WORD into it), hands out fresh integers as the handles of rdx_buffer_create / rdx_buffer_wrap and
    returns 0"""

    def __init__(self):
        self.calls = []
        self._next = 1000

    def _decode(self, a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, C.c_void_p):
            return {"ptr": a.value}
        if hasattr(a, "_obj"):       # C.byref(...)
            obj = a._obj
            if isinstance(obj, C.Structure):
                return "{%s}" % ", ".join(str(getattr(obj, f[0])) for f in obj._fields_)        # the fields' values in the struct's order
            obj.value = OUT_WORD
            return "out"
        return "<%s>" % type(a).__name__

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append([name] + [self._decode(a) for a in args])
            if name in ("rdx_buffer_create", "rdx_buffer_wrap"):
                self._next += 1
                return self._next
            return 0
        return call


@contextlib.contextmanager
def stand_in(rd):
    rec, real = Recorder(), rd._lib.lib
    rd._lib.lib = lambda: rec
    try:
        yield rec
    finally:
        rd._lib.lib = real


def plain(rd, x):
    """a returned value as plain data: a Buffer as its handle and size, a tensor as shape, dtype and device type"""
    if isinstance(x, (tuple, list)):
        return [plain(rd, v) for v in x]
    if isinstance(x, rd.Buffer):
        return "Buffer(%s, %s)" % (x.handle, x.size)
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if hasattr(x, "data_ptr"):
        return "%s %s %s" % (x.device.type, str(x.dtype).replace("torch.", ""), list(x.shape))
    return "<%s>" % type(x).__name__


def outcome(rd, thunk, labels=None):
    """labels: (args, returned) -> {device address: label}, applied to the recorded pointers once the call is over"""
    with stand_in(rd) as rec:
        try:
            ret = thunk()
            out = {"returned": plain(rd, ret)}
        except rd.RadianceError as e:
            ret, out = None, {"refused": str(e)}
        except Exception as e:      # what Python itself refuses (int("x"), a missing attribute): its type is behaviour, its text Python's
            ret, out = None, {"error": type(e).__name__}
    names = labels(ret) if labels else {}
    arg = lambda a: "@" + names.get(a["ptr"], "other") if isinstance(a, dict) else str(a)
    out["calls"] = ["%s(%s)" % (call[0], ", ".join(arg(a) for a in call[1:])) for call in rec.calls]      # one call, one line of text
    return out


# ---- the Buffer route -------------------------------------------------------------------------------------------------------------------
SCALARS = dict(n=5, kind=2, light=3, index=2, max_depth=4, light_count=3, area_count=2, stream=9, frame_id=6, total_samples=8, first_pixel=3, tmin=0.25,
               tmax=50.0, compact=False, debug=False)
BAD_SCALARS = dict(n=(-1, True, 1.5, "3", None), max_depth=(-1, True, 1.5, None, 63), light_count=(-1, True, 1.5, None, 6, 17), area_count=(-1, True, 1.5, None, 15),
                   index=(-1, True, 1.5, None), stream=(-1, True, 1.5, 0xffff), light=(-1, 5, None, "x"))
ONE_BAD = dict(n=-1, max_depth=-1, light_count=99, area_count=-1, index=-1, stream=-1, light=9)      # the one wrong value of each in _order_of_the_checks


def surface_tuple(rd):
    return tuple(rd.Buffer(101 + k, 256) for k in range(4))


def shading_tuple(rd):
    return tuple(rd.Buffer(201 + k, 256) for k in range(7)) + (rd.Sampler(208, 0x1133, 0x1141),)


def good(rd, name):
    """an accepted argument set of the Buffer-route call `name`, by parameter name: a Buffer of its own handle in every buffer
    position (outputs included), a distinct non-zero multiple of 16 as every offset, keys given and randoms None"""
    a = {}
    for k, p in enumerate(inspect.signature(getattr(rd, name)).parameters):
        if p.endswith("_offset"):
            a[p] = 16 * (k + 1)
        elif p in SCALARS:
            a[p] = SCALARS[p]
        elif p == "scene_buffers":
            a[p] = surface_tuple(rd) if name == "ResolveHits" else shading_tuple(rd)
        elif p == "randoms":
            a[p] = None
        else:
            a[p] = rd.Buffer(11 + k, 4096)
    return a


CREATED = {"QueryRays": dict(hits=None), "ResolveHits": dict(out=None), "ResolveMaterials": dict(out=None),
           "ShadeHits": dict(shade=None, next=True, shadow=True, src=None, compact=True), "LightHits": dict(lit=None, shadow=True),
           "ScatterHits": dict(scatter=None, next=None, src=None, compact=True), "GenerateRays": dict(rays=None, keys=True), "Accumulate": dict(),
           "TracePaths": dict(radiance=None, hits=True), "TraceLightPaths": dict(radiance=None), "PunctualLightHits": dict(lit=None, shadow=True),
           "TracePunctualPaths": dict(radiance=None), "AreaLightHits": dict(lit=None, shadow=True), "TraceAreaPaths": dict(radiance=None)}
_RANDOMS = "a Buffer in the place of randoms"
MARSHAL = {        # per call: changes to good(); CREATED[name] (every output created) and n = 0 / a numpy integer are added to each list
    "QueryRays": [dict(kind=1)],
    "ResolveHits": [dict(scene_buffers="no uv"), dict(scene_buffers="object")],
    "ShadeHits": [dict(next=None, shadow=None), dict(next=False, shadow=False), dict(next=True), dict(shadow=True), dict(src=None), dict(src=None, compact=True),
                  dict(compact=True), dict(shade=None), dict(scene_buffers="six"), dict(scene_buffers="no uv"), dict(scene_buffers="object")],
    "ResolveMaterials": [dict(scene_buffers="six"), dict(scene_buffers="no uv")],
    "LightHits": [dict(shadow=None), dict(shadow=False), dict(lit=None), dict(light=0), dict(light=4)],
    "ScatterHits": [dict(keys=None, randoms=_RANDOMS), dict(src=None), dict(src=None, compact=True), dict(compact=True), dict(scatter=None), dict(next=None)],
    "GenerateRays": [dict(pixels=None), dict(seeds=None), dict(pixels=None, seeds=None, keys=None), dict(keys=False), dict(rays=None), dict(keys=True)],
    "Accumulate": [dict(image=None), dict(pixels=None), dict(debug=True), dict(image=None, pixels=None)],
    "TracePaths": [dict(hits=None), dict(hits=False), dict(hits=True), dict(radiance=None), dict(max_depth=0)],
    "TraceLightPaths": [dict(light_count=0), dict(light_count=5)],
    "PunctualLightHits": [dict(shadow=None), dict(shadow=False), dict(lit=None), dict(index=0)],
    "TracePunctualPaths": [dict(light_count=0), dict(light_count=16)],
    "AreaLightHits": [dict(keys=None, randoms=_RANDOMS), dict(stream=None), dict(keys=None, randoms=_RANDOMS, stream=None), dict(shadow=None), dict(shadow=False),
                      dict(lit=None), dict(stream=0xfffe)],
    "TraceAreaPaths": [dict(lights=None, light_count=0), dict(area=None, area_count=0), dict(lights=None, light_count=0, area=None, area_count=0),
                       dict(light_count=14, area_count=2), dict(light_count=0, area_count=0)],
}


def _changed(rd, name, changes):
    a = good(rd, name)
    for p, v in changes.items():
        if v is _RANDOMS:
            v = rd.Buffer(77, 4096)
        elif p == "scene_buffers" and isinstance(v, str):
            t = a[p]
            if v == "no uv":
                v = tuple(None if k == (2 if name == "ResolveHits" else 3) else b for k, b in enumerate(t))
            elif v == "six":
                v = t[:6]
            elif v == "object":
                v = (rd.SurfaceBuffers if name == "ResolveHits" else rd.ShadingBuffers)(*t)
        a[p] = v
    return a


def _call(rd, name, a):
    return lambda: getattr(rd, name)(**a)


def marshal_cases(rd):
    for name in BUFFER_ROUTE:
        rows = [dict(), CREATED[name], dict(CREATED[name], n=np.uint32(0)), dict(n=np.int64(5))] + MARSHAL[name]
        for k, changes in enumerate(rows):
            yield "marshal/%s/%d" % (name, k), _call(rd, name, _changed(rd, name, changes))


def _single_faults(rd, name):
    """(label, changes) of one fault each: no Buffer in each buffer position (an int, and None where the position has no default),
    each bad scalar, each bad scene_buffers, both and neither of keys and randoms"""
    a = good(rd, name)
    sig = inspect.signature(getattr(rd, name)).parameters
    for p, v in a.items():
        if isinstance(v, rd.Buffer) or p == "randoms":
            yield "%s=5" % p, {p: 5}
            if isinstance(v, rd.Buffer) and sig[p].default is inspect.Parameter.empty:
                yield "%s=None" % p, {p: None}
        elif p in BAD_SCALARS:
            for bad in BAD_SCALARS[p]:
                yield "%s=%r" % (p, bad), {p: bad}
        elif p == "scene_buffers":
            t = a[p]
            yield "scene_buffers=5", {p: 5}
            yield "scene_buffers=(1, 2)", {p: (1, 2)}
            yield "scene_buffers=nine", {p: t + t[:9 - len(t)]}
            yield "scene_buffers=()", {p: ()}
            for k in range(len(t)):
                yield "scene_buffers[%d]=5" % k, {p: t[:k] + (5,) + t[k + 1:]}
                if k < 6:
                    yield "scene_buffers[%d]=None" % k, {p: t[:k] + (None,) + t[k + 1:]}
            if len(t) == 8:
                yield "scene_buffers.sampler=a Buffer", {p: t[:7] + (t[0],)}
    for p in CREATED[name]:         # every output position as True and as False, whether or not the call takes them there
        if p != "compact":
            yield "%s=True" % p, {p: True}
            yield "%s=False" % p, {p: False}
    if "randoms" in a:
        yield "both", {"randoms": _RANDOMS}
        yield "neither", {"keys": None}
    if name == "TraceAreaPaths":
        yield "lights=None,count=3", {"lights": None}
        yield "area=None,count=2", {"area": None}
        yield "sum=17", {"light_count": 9, "area_count": 8}
        yield "sum=17,lights=None", {"light_count": 0, "area_count": 17, "lights": None}


def _order_of_the_checks(rd, name):
    """every parameter wrong at once, then mended one by one: at each step the parameter is mended whose mending changes what the
    call says (the first in the signature, if none does), so the texts come out in the order of the checks.  A parameter may be
    wrong in more than one way, mended one way at a time.  -> [parameter mended, what the call said before], ..., the end state"""
    a = good(rd, name)
    wrong = {}
    for p, v in a.items():
        if p == "keys" and "randoms" in a:
            wrong[p] = [5, None]            # no Buffer; then none, with randoms None: neither
        elif isinstance(v, rd.Buffer) or p == "randoms":
            wrong[p] = [5]
        elif p in ONE_BAD:
            wrong[p] = [ONE_BAD[p]]
        elif p == "scene_buffers":
            wrong[p] = [(1, 2), v[:1] + (5,) + v[2:]]
    said = lambda state: {k: v for k, v in outcome(rd, _call(rd, name, dict(a, **{p: ways[0] for p, ways in state.items()}))).items() if k != "calls"}
    steps = []
    while wrong:
        now = said(wrong)
        if "refused" not in now:        # what is still wrong is not looked at (a negative n of a per-hit call)
            break
        mended = {p: {q: (w[1:] if q == p else w) for q, w in wrong.items() if q != p or len(w) > 1} for p in wrong}
        p = next((p for p in wrong if said(mended[p]) != now), next(iter(wrong)))
        if steps and steps[-1][1] == now["refused"]:
            steps[-1][0] += ", " + p            # one check that looks at several parameters
        else:
            steps.append([p, now["refused"]])
        wrong = mended[p]
    return steps + [["still wrong: " + ", ".join(wrong)] + list(said(wrong).items())[0:1]]


def refusal_cases(rd):
    for name in BUFFER_ROUTE:
        for label, changes in _single_faults(rd, name):
            yield "refuse/%s/%s" % (name, label), _call(rd, name, _changed(rd, name, changes))
        yield "order/%s" % name, (lambda name=name: _order_of_the_checks(rd, name))


# ---- the torch route --------------------------------------------------------------------------------------------------------------------
class T:
    """a tensor argument: `cols` columns (None: one-dimensional) of dtype "f" / "i" / "u8", `rows` rows (None: the call's n)"""

    def __init__(self, cols, dtype="f", rows=None):
        self.cols, self.dtype, self.rows = cols, dtype, rows


TABLE = 2       # records of a light table
TORCH = {       # per call: (parameter, T or a plain value) in the order of its signature; "tlas" / "buf" / "shading" / "surface" are made per case
    "QueryRaysTorch": [("tlas", "tlas"), ("rays_tensor", T(8)), ("kind", 1), ("out", T(8, "i"))],
    "ResolveHitsTorch": [("tlas", "tlas"), ("rays_tensor", T(8)), ("hits_tensor", T(8, "i")), ("scene_buffers", "surface"), ("out", T(16))],
    "ShadeHitsTorch": [("tlas", "tlas"), ("rays_t", T(8)), ("hits_t", T(8, "i")), ("keys_t", T(4, "i")), ("scene_buffers", "shading"), ("compact", True),
                       ("sample_next", True)],
    "ResolveMaterialsTorch": [("tlas", "tlas"), ("rays_tensor", T(8)), ("hits_tensor", T(8, "i")), ("scene_buffers", "shading"), ("out", T(16))],
    "LightHitsTorch": [("rays_t", T(8)), ("materials_t", T(16)), ("scene_buffer", "buf"), ("light", 3), ("want_shadow", True)],
    "ScatterHitsTorch": [("rays_t", T(8)), ("materials_t", T(16)), ("surfaces_t", T(16)), ("keys_t", T(4, "i")), ("randoms_t", None), ("compact", True)],
    "GenerateRaysTorch": [("camera", "buf"), ("n_or_pixels", T(None, "i")), ("frame_id", 6), ("total_samples", 8), ("seeds", T(4, "i"))],
    "AccumulateTorch": [("colors", T(4)), ("frame_id", 6), ("scratch", T(4, "f", 6)), ("image", T(4, "u8", 6)), ("pixels", T(None, "i")), ("debug", False)],
    "TracePathsTorch": [("tlas", "tlas"), ("rays_t", T(8)), ("keys_t", T(4, "i")), ("max_depth", 4), ("scene_buffers", "shading"), ("want_hits", False)],
    "TraceLightPathsTorch": [("tlas", "tlas"), ("rays_t", T(8)), ("keys_t", T(4, "i")), ("max_depth", 4), ("light_count", 3), ("scene_buffers", "shading")],
    "PunctualLightHitsTorch": [("rays_t", T(8)), ("materials_t", T(16)), ("lights_t", T(16, "f", TABLE)), ("index", 1), ("want_shadow", True)],
    "TracePunctualPathsTorch": [("tlas", "tlas"), ("rays_t", T(8)), ("keys_t", T(4, "i")), ("max_depth", 4), ("lights_t", T(16, "f", TABLE)),
                                ("scene_buffers", "shading")],
    "AreaLightHitsTorch": [("rays_t", T(8)), ("materials_t", T(16)), ("area_t", T(16, "f", TABLE)), ("index", 1), ("keys", T(4, "i")), ("randoms", None),
                           ("stream", 9), ("want_shadow", True)],
    "TraceAreaPathsTorch": [("tlas", "tlas"), ("rays_t", T(8)), ("keys_t", T(4, "i")), ("max_depth", 4), ("lights_t", T(16, "f", TABLE)),
                            ("area_t", T(16, "f", TABLE)), ("scene_buffers", "shading")],
}
_BUF, _FRAME = "a Buffer", "a Buffer of a frame"
TORCH_VARIANTS = {      # accepted calls: changes to the base; each runs at 3 rows (marshalling) and at 0 rows (the returned structure)
    "QueryRaysTorch": [dict(out=None), dict(kind=2, out=T(8))],
    "ResolveHitsTorch": [dict(out=None), dict(hits_tensor=T(8))],
    "ShadeHitsTorch": [dict(compact=False), dict(sample_next=False), dict(compact=False, sample_next=False)],
    "ResolveMaterialsTorch": [dict(out=None)],
    "LightHitsTorch": [dict(want_shadow=False)],
    "ScatterHitsTorch": [dict(keys_t=None, randoms_t=T(4)), dict(compact=False)],
    "GenerateRaysTorch": [dict(seeds=None), dict(n_or_pixels="n"), dict(n_or_pixels="n", seeds=None), dict(n_or_pixels="numpy n")],
    "AccumulateTorch": [dict(image=None), dict(pixels=None), dict(scratch=_FRAME, image=_FRAME), dict(debug=True), dict(scratch=T(4, "f", 0)),
                        dict(image=T(4, "u8", 0))],
    "TracePathsTorch": [dict(want_hits=True), dict(max_depth=0)],
    "TraceLightPathsTorch": [dict(light_count=0)],
    "PunctualLightHitsTorch": [dict(want_shadow=False), dict(index=0)],
    "TracePunctualPathsTorch": [dict(lights_t=T(16, "f", 0)), dict(lights_t=T(16, "f", 16))],
    "AreaLightHitsTorch": [dict(keys=None, randoms=T(4)), dict(stream=None), dict(keys=None, randoms=T(4), stream=None), dict(want_shadow=False)],
    "TraceAreaPathsTorch": [dict(lights_t=None), dict(area_t=None), dict(lights_t=None, area_t=None), dict(lights_t=T(16, "f", 0)), dict(area_t=T(16, "f", 0)),
                            dict(lights_t=T(16, "f", 14))],
}
TORCH_FAULTS = {        # the faults of the arguments that are no tensors, and of tensors that the rules above do not reach
    "QueryRaysTorch": [dict(tlas=5)],
    "ResolveHitsTorch": [dict(tlas=5), dict(scene_buffers=5), dict(scene_buffers=(1, 2))],
    "ShadeHitsTorch": [dict(tlas=5), dict(scene_buffers=5)],
    "ResolveMaterialsTorch": [dict(tlas=5), dict(scene_buffers=(1, 2))],
    "LightHitsTorch": [dict(scene_buffer=5), dict(scene_buffer=None), dict(light=5), dict(light=-1), dict(light="x"), dict(scene_buffer=5, light=9)],
    "ScatterHitsTorch": [dict(keys_t=None), dict(randoms_t=T(4)), dict(keys_t=None, randoms_t=T(4, "i")), dict(keys_t=None, randoms_t=T(3))],
    "GenerateRaysTorch": [dict(n_or_pixels=-1), dict(n_or_pixels=True), dict(n_or_pixels=1.5), dict(n_or_pixels="x"), dict(n_or_pixels=None), dict(camera=5),
                          dict(n_or_pixels="n", seeds=T(4, "i", 4))],
    "AccumulateTorch": [dict(scratch=None), dict(scratch=T(4, "u8", 6)), dict(scratch=T(3, "f", 6)), dict(scratch=5), dict(image=T(4, "f", 6)), dict(image=T(3, "u8", 6)),
                        dict(image=5), dict(scratch="cpu"), dict(image="cpu"), dict(scratch=None, pixels=T(None, "f"))],
    "TracePathsTorch": [dict(max_depth=-1), dict(max_depth=True), dict(max_depth=1.5), dict(max_depth=63), dict(tlas=5), dict(scene_buffers=5)],
    "TraceLightPathsTorch": [dict(max_depth=-1), dict(max_depth=True), dict(light_count=6), dict(light_count=-1), dict(light_count=True), dict(light_count=1.5),
                             dict(max_depth=-1, light_count=6), dict(tlas=5)],
    "PunctualLightHitsTorch": [dict(index=2), dict(index=-1), dict(index=1.5), dict(index=True), dict(lights_t=T(16, "f", 0), index=0)],
    "TracePunctualPathsTorch": [dict(lights_t=T(16, "f", 17)), dict(max_depth=-1), dict(max_depth=-1, lights_t=T(16, "f", 17)), dict(lights_t=None), dict(tlas=5)],
    "AreaLightHitsTorch": [dict(index=2), dict(index=-1), dict(index=1.5), dict(keys=None), dict(randoms=T(4)), dict(stream=0xffff), dict(stream=-1), dict(stream=True),
                           dict(index=2, stream=-1), dict(keys=None, index=-1), dict(keys=None, randoms=T(3))],
    "TraceAreaPathsTorch": [dict(lights_t=T(16, "f", 15)), dict(lights_t=T(16, "f", 17), area_t=None), dict(max_depth=-1), dict(max_depth=True),
                            dict(max_depth=-1, lights_t=T(16, "f", 15)), dict(tlas=5), dict(scene_buffers=(1, 2))],
}
_NP = {"f": np.float32, "i": np.int32, "u8": np.uint8}


def _torch_args(rd, torch, name, n, changes, device):
    """the arguments of one torch-route call by name, and the tensors among them (for the labels of their addresses)"""
    dt = {"f": torch.float32, "i": torch.int32, "u8": torch.uint8}
    a = {}
    for p, v in TORCH[name]:
        v = changes.get(p, v)
        if isinstance(v, T):
            rows = n if v.rows is None else v.rows
            v = torch.zeros((rows,) if v.cols is None else (rows, v.cols), dtype=dt[v.dtype], device=device)
        elif v == "tlas":
            v = rd.Buffer(1, 64)
        elif v == "buf":
            v = rd.Buffer(2, 256)
        elif v is _FRAME:
            v = rd.Buffer(3 if p == "scratch" else 4, 96)
        elif v == "shading":
            v = shading_tuple(rd)
        elif v == "surface":
            v = surface_tuple(rd)
        elif v == "n":
            v = n
        elif v == "numpy n":
            v = np.int64(n)
        elif v == "cpu":
            v = torch.zeros((6, 4), dtype=torch.float32 if p == "scratch" else torch.uint8)
        a[p] = v
    return a


def _torch_case(rd, torch, name, a):
    def labels(ret):
        names = {}
        for k, t in enumerate(ret if isinstance(ret, (tuple, list)) else [ret]):
            if hasattr(t, "data_ptr") and t.numel():
                names[t.data_ptr()] = "returned[%d]" % k
        for p, t in a.items():
            if hasattr(t, "data_ptr") and t.numel():
                names[t.data_ptr()] = p
        return names
    return (lambda: getattr(rd, name)(**a)), labels


TENSOR_FAULTS = ("dtype", "trailing", "rows", "strided", "cpu", "numpy")


def _tensor_faults(torch, t):
    """one tensor position, each way it can be wrong"""
    rows, cols = t.shape[0], (t.shape[1] if t.dim() == 2 else None)
    shape = lambda r, c: (r,) if c is None else (r, c)
    yield "dtype", t.double()
    yield "trailing", torch.zeros((rows, 2) if cols is None else (rows, cols + 1), dtype=t.dtype, device=t.device)
    yield "rows", torch.zeros(shape(rows + 1, cols), dtype=t.dtype, device=t.device)
    yield "strided", torch.zeros((2 * rows,) if cols is None else (rows, 2 * cols), dtype=t.dtype, device=t.device)[..., ::2]
    yield "cpu", t.cpu()
    yield "numpy", np.zeros(tuple(t.shape), np.float32)


def torch_cases(rd, torch, device="cuda"):
    """(id, thunk, labels) of the torch route on tensors of `device`: accepted calls at 3 and at 0 rows, every tensor position wrong
    in each way, the other arguments' faults"""
    for name in TORCH_ROUTE:
        for k, changes in enumerate([dict()] + TORCH_VARIANTS[name]):
            for n in (3, 0):
                yield ("torch/%s/%d/n=%d" % (name, k, n),) + _torch_case(rd, torch, name, _torch_args(rd, torch, name, n, changes, device))
        for base_no, base in enumerate([dict()] + [v for v in TORCH_VARIANTS[name] if any(isinstance(x, T) for x in v.values())]):
            a = _torch_args(rd, torch, name, 3, base, device)
            for p, t in a.items():
                if hasattr(t, "data_ptr") and (base_no == 0 or p in base):
                    for label, bad in _tensor_faults(torch, t):
                        yield ("torch-refuse/%s/%d/%s/%s" % (name, base_no, p, label),) + _torch_case(rd, torch, name, dict(a, **{p: bad}))
        for k, changes in enumerate(TORCH_FAULTS[name]):
            yield ("torch-refuse/%s/other/%d" % (name, k),) + _torch_case(rd, torch, name, _torch_args(rd, torch, name, 3, changes, device))


def cpu_tensor_cases(rd, torch):
    """the torch route fed CPU tensors: the first tensor's refusal is reachable without a GPU"""
    for name in TORCH_ROUTE:
        for k, changes in enumerate([dict()] + TORCH_VARIANTS[name]):
            if "n" in changes.values() or "numpy n" in changes.values():       # a count in the place of the first tensor asks torch for a device
                continue
            yield ("cpu-tensors/%s/%d" % (name, k),) + _torch_case(rd, torch, name, _torch_args(rd, torch, name, 3, changes, "cpu"))


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def _hash(text):
    return None if text is None else hashlib.sha256(text.encode()).hexdigest()[:16]


def public_surface(rd):
    """every public name of rd.py as one line: a function's signature and the hash of its docstring; a class's, and under
    Class.member those of its methods; the value of a constant; the size of a dtype and the hash of its fields"""
    signed = lambda f: "%s doc %s" % (inspect.signature(f) if f else None, _hash(f.__doc__) if f else None)
    out = {}
    for name, obj in sorted(vars(rd).items()):
        if name.startswith("_") or inspect.ismodule(obj):
            continue
        if inspect.isclass(obj):
            if obj.__module__ != rd.__name__:
                continue
            out[name] = "%s class doc %s" % (signed(vars(obj).get("__init__")), _hash(obj.__doc__))       # RadianceError has no __init__ of its own
            for m, f in sorted(vars(obj).items()):
                if (inspect.isfunction(f) or isinstance(f, staticmethod)) and m != "__init__":
                    out["%s.%s" % (name, m)] = signed(f.__func__ if isinstance(f, staticmethod) else f)
        elif inspect.isfunction(obj):
            out[name] = signed(obj)
        elif isinstance(obj, np.dtype):
            out[name] = "dtype of %d bytes, fields %s" % (obj.itemsize, _hash(str(obj.descr)))
        else:
            out[name] = repr(obj) if len(repr(obj)) <= 60 else "value %s" % _hash(repr(obj))
    return out


def cpu_part(rd):
    """what is recorded and replayed without a GPU"""
    import torch
    part = {cid: outcome(rd, thunk) for cid, thunk in itertools.chain(marshal_cases(rd), refusal_cases(rd))}
    part.update({cid: outcome(rd, thunk, labels) for cid, thunk, labels in cpu_tensor_cases(rd, torch)})
    return {"cases": part, "surface": public_surface(rd)}


def gpu_part(rd, torch):
    """what needs CUDA tensors"""
    return {"cases": {cid: outcome(rd, thunk, labels) for cid, thunk, labels in torch_cases(rd, torch)}}


def _split(cid):
    parts = cid.split("/", 2)
    return ("/".join(parts[:2]), parts[2]) if len(parts) == 3 else (parts[0], parts[1])


def pack(doc):
    """the golden as it is stored: every distinct outcome once (many cases are refused in the same words), and per part and group
    of cases -- "marshal/QueryRays" -- the number of each case's outcome"""
    short = lambda v: v["refused"] if set(v) == {"refused", "calls"} and not v["calls"] else v       # a refusal before any library call: its text alone
    texts = sorted({json.dumps(short(v), sort_keys=True) for part in ("cpu", "gpu") if part in doc for v in doc[part]["cases"].values()})
    number = {t: k for k, t in enumerate(texts)}
    out = {"recorded_at": doc["recorded_at"], "surface": doc["cpu"]["surface"], "outcomes": [json.loads(t) for t in texts]}
    for part in ("cpu", "gpu"):
        out[part] = {}
        for cid, v in sorted(doc.get(part, {"cases": {}})["cases"].items()):
            group, rest = _split(cid)
            out[part].setdefault(group, {})[rest] = number[json.dumps(short(v), sort_keys=True)]
        for rows in out[part].values():         # a tensor position that is refused alike in each of its six ways is one row, ".../*"
            for stem in sorted({rest.rsplit("/", 1)[0] for rest in rows if "/" in rest}):
                same = {rows.get("%s/%s" % (stem, way)) for way in TENSOR_FAULTS}
                if len(same) == 1 and None not in same:
                    for way in TENSOR_FAULTS:
                        del rows["%s/%s" % (stem, way)]
                    rows[stem + "/*"] = same.pop()
    return out


def unpack(stored):
    """-> {"recorded_at", "cpu": {"cases": {id: outcome}, "surface"}, "gpu": {"cases"}}, what cpu_part and gpu_part return"""
    def cases(part):
        out = {}
        for group, rows in stored[part].items():
            for rest, k in rows.items():
                v = stored["outcomes"][k]
                v = {"refused": v, "calls": []} if isinstance(v, str) else v
                for r in ([rest[:-1] + way for way in TENSOR_FAULTS] if rest.endswith("/*") else [rest]):
                    out["%s/%s" % (group, r)] = v
        return out
    return {"recorded_at": stored["recorded_at"], "cpu": {"cases": cases("cpu"), "surface": stored["surface"]}, "gpu": {"cases": cases("gpu")}}


def golden(path):
    return unpack(json.load(open(path)))


def differences(got, want, limit=12):
    """the ids at which two recorded parts differ, with both sides, for an assertion's message"""
    out = []
    for section in sorted(set(got) | set(want)):
        g, w = got.get(section, {}), want.get(section, {})
        for k in sorted(set(g) | set(w)):
            if g.get(k) != w.get(k):
                out.append("%s %s:\n  got      %r\n  recorded %r" % (section, k, g.get(k), w.get(k)))
    return out[:limit], len(out)
