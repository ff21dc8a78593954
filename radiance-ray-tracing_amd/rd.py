"""rd.py -- Python mirror of the reference's host API `namespace RD`
(radiance/include/radiance.h:86-174), over the C ABI of include/rdx.h.

Same function names, argument order and meaning as the reference, so the tests read like the
reference's own sample (samples/sample1.cpp:363-498).  Differences, all deliberate:

  * errors raise `RadianceError` (the reference prints and calls exit(-1), clcontext.h:27-47;
    the C++ facade in include/radiance.h keeps that behaviour);
  * `Mesh.vertexData` / `indexData` are numpy arrays ((N,3) float32 / (M,3) uint32) instead of
    std::vector<Vec3> / std::vector<Triangle>;
  * buffers accept numpy arrays or bytes for `data`.
"""
import ctypes as C

import numpy as np

from . import _lib

CHANNEL = 4
RD_CHANNEL = CHANNEL

# enum DescriptorType (radiance.h:21-29)
ACCEL_STRUCT_TYPE, IMAGE_TYPE, IMAGE_ARRAY_TYPE, IMAGE_SAMPLER_TYPE, BUFFER_TYPE, TEX_ARRAY_TYPE = range(6)

# addressing / filter modes keep the OpenCL values the reference forwards (radiance.h:94-112)
RD_ADDRESS_CLAMP_TO_EDGE, RD_ADDRESS_CLAMP, RD_ADDRESS_REPEAT, RD_ADDRESS_MIRRORED_REPEAT = 0x1131, 0x1132, 0x1133, 0x1134
RD_FILTER_NEAREST, RD_FILTER_LINEAR = 0x1140, 0x1141


class RadianceError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise RadianceError(_lib.last_error())


def _handle(h, what):
    if not h:
        raise RadianceError("%s: %s" % (what, _lib.last_error()))
    return h


# ---- POD structs (radiance/src/core.h:103-158) as numpy dtypes ----------------------------------
RayTraceProperties = np.dtype([("totalSamples", "<u4"), ("batchSize", "<u4"), ("depth", "<u4"), ("debug", "<u4")])
Material = np.dtype([("albedo", "<f4", 4), ("metallic", "<f4"), ("roughness", "<f4"), ("transmission", "<f4"),
                     ("ior", "<f4"), ("albedoTexIdx", "<i4"), ("metallicTexIdx", "<i4"),
                     ("roughnessTexIdx", "<i4"), ("normalTexIdx", "<i4")])
MeshInfo = np.dtype([("vertexOffset", "<i4"), ("indexOffset", "<i4"), ("uvOffset", "<i4"), ("normalOffset", "<i4"),
                     ("materialIndex", "<i4"), ("_0", "<i4"), ("_1", "<i4"), ("_2", "<i4")])
DirLight = np.dtype([("direction", "<f4", 4), ("color", "<f4", 4)])
SceneProperties = np.dtype([("lightCount", "<u4", 4), ("lights", DirLight, 5)])
PhysicalCamera = np.dtype([("widthPixel", "<f4"), ("heightPixel", "<f4"), ("focalLength", "<f4"),
                           ("sensorWidth", "<f4"), ("focalDistance", "<f4"), ("fStop", "<f4"),
                           ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4")])
assert (RayTraceProperties.itemsize, Material.itemsize, MeshInfo.itemsize, DirLight.itemsize,
        SceneProperties.itemsize, PhysicalCamera.itemsize) == (16, 48, 32, 32, 176, 48)


class Mesh:
    """struct Mesh (radiance.h:44-48)"""

    def __init__(self, vertexData=None, indexData=None):
        self.vertexData = np.zeros((0, 3), np.float32) if vertexData is None else vertexData
        self.indexData = np.zeros((0, 3), np.uint32) if indexData is None else indexData


class BottomAccelStruct:
    def __init__(self, handle):
        self.handle = handle

    @property
    def data(self):
        """the host blob (struct _BottomAccelStruct::data, radiance.h:52-58)"""
        n = C.c_uint32(0)
        p = _lib.lib().rdx_blas_data(self.handle, C.byref(n))
        return bytes((C.c_uint8 * n.value).from_address(p))

    @property
    def max_depth(self):
        return _lib.lib().rdx_blas_max_depth(self.handle)


class Instance:
    """struct Instance (radiance.h:64-74); transform is a row-major 4x4"""

    def __init__(self, transform=None, SBTOffset=0, customInstanceID=0, bottomAccelStruct=None):
        self.transform = np.eye(4, dtype=np.float32) if transform is None else np.asarray(transform, np.float32).reshape(4, 4)
        self.SBTOffset = SBTOffset
        self.customInstanceID = customInstanceID
        self.bottomAccelStruct = bottomAccelStruct


class Buffer:
    """RD::Buffer / Image / TopAccelStruct (all `cl_mem` in the reference, radiance.h:12-19)"""

    def __init__(self, handle, size, keepalive=None):
        self.handle = handle
        self.size = size
        self._keepalive = keepalive     # e.g. the torch tensor whose memory is wrapped

    @property
    def device_ptr(self):
        return _lib.lib().rdx_buffer_device_ptr(self.handle)


class PipelineCreateInfo:
    """struct PipelineCreateInfo (radiance.h:81-88)"""

    def __init__(self, maxRayRecursionDepth=1, layout=(), modules=(), groups=()):
        self.maxRayRecursionDepth = maxRayRecursionDepth
        self.layout = list(layout)
        self.modules = list(modules)
        self.groups = list(groups)


class Platform:
    """struct Platform (radiance.h:146-174): process-wide singleton owning the device and stream."""
    _instance = None

    def __init__(self):
        self.activePipeline = None
        self.initialized = False

    @staticmethod
    def GetPlatform(device=-1):
        if Platform._instance is None:
            Platform._instance = Platform()
        p = Platform._instance
        if not p.initialized:
            _check(_lib.lib().rdx_init(device))
            p.initialized = True
        return p

    @staticmethod
    def InitDevices(n, ordinals=None):
        """Extension: render every TraceRays frame on `n` devices from this one process (rdx_init_devices); call before any
        buffer is created.  Returns the platform."""
        p = Platform.GetPlatform(-1 if ordinals is None else ordinals[0])
        arr = (C.c_int * n)(*ordinals) if ordinals is not None else None
        _check(_lib.lib().rdx_init_devices(int(n), arr))
        return p

    @staticmethod
    def device_name():
        buf = C.create_string_buffer(256)
        _check(_lib.lib().rdx_device_name(buf, 256))
        return buf.value.decode()


def _as_bytes_ptr(data, size):
    if isinstance(data, np.ndarray):
        arr = np.ascontiguousarray(data)
        if arr.nbytes < size:
            raise RadianceError("host array (%d bytes) smaller than the requested transfer (%d)" % (arr.nbytes, size))
        return arr, arr.ctypes.data
    if isinstance(data, (bytes, bytearray)):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
        if len(data) < size:
            raise RadianceError("host bytes smaller than the requested transfer")
        return buf, C.addressof(buf)
    raise TypeError("data must be a numpy array or bytes")


# ---- acceleration structures (radiance.h:88-92) ---------------------------------------------------
def BuildAccelStruct(platform, what):
    """Both overloads of RD::BuildAccelStruct: Mesh -> BottomAccelStruct, [Instance] -> TopAccelStruct."""
    L = _lib.lib()
    if isinstance(what, Mesh):
        v = np.ascontiguousarray(what.vertexData, np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(what.indexData, np.uint32).reshape(-1, 3)
        h = L.rdx_blas_build(v.ctypes.data, v.shape[0], i.ctypes.data, i.shape[0])
        return BottomAccelStruct(_handle(h, "BuildAccelStruct(Mesh)"))
    insts = list(what)
    arr = _instance_array(insts)
    h = L.rdx_tlas_build(arr, len(insts))
    _handle(h, "BuildAccelStruct(instances)")
    return Buffer(h, L.rdx_buffer_size(h))


def BuildAccelStructs(platform, meshes):
    """[Mesh] -> [BottomAccelStruct], built concurrently inside the library (rdx_blas_build_many); same results as
    BuildAccelStruct(platform, mesh) for each mesh in turn."""
    L = _lib.lib()
    meshes = list(meshes)
    n = len(meshes)
    if n == 0:
        return []
    vs = [np.ascontiguousarray(m.vertexData, np.float32).reshape(-1, 3) for m in meshes]
    ts = [np.ascontiguousarray(m.indexData, np.uint32).reshape(-1, 3) for m in meshes]
    vp = (C.c_void_p * n)(*[v.ctypes.data for v in vs])
    tp = (C.c_void_p * n)(*[t.ctypes.data for t in ts])
    nv = (C.c_uint32 * n)(*[v.shape[0] for v in vs])
    nt = (C.c_uint32 * n)(*[t.shape[0] for t in ts])
    out = (C.c_void_p * n)()
    _check(L.rdx_blas_build_many(n, vp, nv, tp, nt, out))
    return [BottomAccelStruct(_handle(out[i], "BuildAccelStructs")) for i in range(n)]


def _instance_array(instances):
    arr = (_lib.rdx_instance * max(len(instances), 1))()
    for k, inst in enumerate(instances):
        m = np.asarray(inst.transform, np.float32).reshape(16)
        for j in range(16):
            arr[k].transform[j] = float(m[j])
        arr[k].SBTOffset = inst.SBTOffset
        arr[k].customInstanceID = inst.customInstanceID
        arr[k].bottomAccelStruct = inst.bottomAccelStruct.handle if inst.bottomAccelStruct else None
    return arr


def UpdateAccelStruct(platform, tlas, instances):
    """Extension (rdx_tlas_update): other transforms / SBT offsets / custom ids for the instances `tlas` was built from -- same
    count, same BLAS at every index.  Afterwards `tlas` holds what BuildAccelStruct(platform, instances) would have built; the
    Buffer stays bound, its `size` (refreshed here) and `device_ptr` may change."""
    if not isinstance(tlas, Buffer):
        raise RadianceError("UpdateAccelStruct: tlas must be the Buffer BuildAccelStruct returned")
    L = _lib.lib()
    insts = list(instances)
    _check(L.rdx_tlas_update(tlas.handle, _instance_array(insts), len(insts)))
    tlas.size = L.rdx_buffer_size(tlas.handle)
    return tlas


def GetTlasUpdateStats():
    """rdx_tlas_update_stats of the last UpdateAccelStruct: path (0 blob only, 1 incremental, 2 full re-derivation), top-level
    node counts, bytes moved, owner words rewritten, host / device milliseconds"""
    st = _lib.rdx_tlas_update_stats()
    _check(_lib.lib().rdx_get_tlas_update_stats(C.byref(st)))
    return st


def BuildTopAccelStructBlob(instances):
    """Host-only TLAS build (no GPU): returns (blob bytes, max depth).  Extension used by the CPU tests."""
    L = _lib.lib()
    instances = list(instances)
    arr = _instance_array(instances)
    n, d = C.c_uint32(0), C.c_int(0)
    p = L.rdx_tlas_build_blob(arr, len(instances), C.byref(n), C.byref(d))
    _handle(p, "BuildAccelStruct(instances)")
    blob = bytes((C.c_uint8 * n.value).from_address(p))
    L.rdx_free(p)
    return blob, d.value


def TopAccelStructToFile(platform, accelStruct, path):
    _check(_lib.lib().rdx_tlas_to_file(accelStruct.handle, str(path).encode()))


def FileToTopAccelStruct(platform, path):
    """The reference returns through an out-parameter (radiance.h:92); here the handle is returned."""
    L = _lib.lib()
    h = _handle(L.rdx_tlas_from_file(str(path).encode()), "FileToTopAccelStruct")
    return Buffer(h, L.rdx_buffer_size(h))


# ---- resources (radiance.h:115-128) ----------------------------------------------------------------
def CreateBuffer(platform, size):
    h = _handle(_lib.lib().rdx_buffer_create(int(size)), "CreateBuffer")
    return Buffer(h, int(size))


def CreateImage(platform, width, height):
    """radiance.cpp:86-93: an RGBA8 image is a width*height*4-byte buffer"""
    return CreateBuffer(platform, int(width) * int(height) * CHANNEL)


class Sampler:
    def __init__(self, handle, addressingMode, filterMode):
        self.handle, self.addressingMode, self.filterMode = handle, addressingMode, filterMode


def CreateImageArray(platform, width, height, arraySize):
    """radiance.cpp:96-120: `arraySize` RGBA8 images of width x height (CL_RGBA / CL_UNSIGNED_INT8)"""
    h = _handle(_lib.lib().rdx_image_array_create(int(width), int(height), int(arraySize)), "CreateImageArray")
    b = Buffer(h, int(width) * int(height) * int(arraySize) * 4)
    b.width, b.height, b.arraySize = int(width), int(height), int(arraySize)
    return b


def CreateSampler(platform, addressingMode, filterMode):
    """radiance.cpp:122-130 (normalized coordinates)"""
    return Sampler(_handle(_lib.lib().rdx_sampler_create(int(addressingMode), int(filterMode)), "CreateSampler"), addressingMode, filterMode)


def WriteImage(platform, handle, width, height, arrayIndex, data):
    """radiance.cpp:214-224: the (width, height) region at the origin of layer `arrayIndex`, RGBA8, rows tightly packed"""
    keep, ptr = _as_bytes_ptr(data, int(width) * int(height) * 4)
    _check(_lib.lib().rdx_image_write(handle.handle, int(width), int(height), int(arrayIndex), ptr))


def ReadImage(platform, handle, width, height, arrayIndex, data=None):
    """radiance.cpp:202-212"""
    if data is None:
        data = np.empty((int(height), int(width), 4), np.uint8)
    _check(_lib.lib().rdx_image_read(handle.handle, int(width), int(height), int(arrayIndex), data.ctypes.data))
    return data


def WrapDeviceMemory(platform, device_ptr, size, keepalive=None):
    """Extension: adopt device memory owned by the caller (e.g. a torch tensor) as an RD::Buffer."""
    h = _handle(_lib.lib().rdx_buffer_wrap(C.c_void_p(int(device_ptr)), int(size)), "WrapDeviceMemory")
    return Buffer(h, int(size), keepalive)


def WriteBuffer(platform, handle, size, data, offset=0):
    keep, ptr = _as_bytes_ptr(data, size)
    _check(_lib.lib().rdx_buffer_write(handle.handle, int(offset), int(size), ptr))


def ReadBuffer(platform, handle, size, data=None, offset=0):
    """Reads `size` bytes; fills `data` (numpy array) if given and returns it, else returns bytes-like uint8 array."""
    if data is None:
        data = np.empty(int(size), np.uint8)
    if not data.flags["C_CONTIGUOUS"] or data.nbytes < size:
        raise RadianceError("ReadBuffer: destination must be C-contiguous and large enough")
    _check(_lib.lib().rdx_buffer_read(handle.handle, int(offset), int(size), data.ctypes.data))
    return data


# ---- pipeline (radiance.h:130-144) -------------------------------------------------------------------
def CreateDescriptorSet(handles):
    return list(handles)


def CreatePipelineLayout(descriptorTypes):
    return list(descriptorTypes)


def CreateShaderModule(platform, code, size, name):
    if isinstance(code, str):
        code = code.encode()
    h = _handle(_lib.lib().rdx_shader_module_create(code, int(size), name.encode() if isinstance(name, str) else name),
                "CreateShaderModule")
    return h


def SetShaderIncludePath(path):
    """-I directory for user shader programs (the reference's SHADER_LIB_PATH, radiance.h:7)"""
    _check(_lib.lib().rdx_shader_include_path(str(path).encode() if path else None))


def CreatePipeline(pipelineCreateInfo):
    return pipelineCreateInfo


def BindPipeline(platform, pipeline):
    platform.activePipeline = pipeline
    if not pipeline.modules:
        raise RadianceError("BindPipeline: pipeline has no shader module")
    _check(_lib.lib().rdx_bind_pipeline(pipeline.modules[0]))


def BindDescriptorSet(platform, descriptorSet):
    n = len(descriptorSet)
    arr = (C.c_void_p * max(n, 1))()
    for i, h in enumerate(descriptorSet):
        arr[i] = h.handle if isinstance(h, (Buffer, Sampler)) else None
    _check(_lib.lib().rdx_bind_descriptor_set(arr, n))


def TraceRays(platform, raygenGroupIndex, missGroupIndex, hitGroupIndex, width, height):
    _check(_lib.lib().rdx_trace_rays(raygenGroupIndex, missGroupIndex, hitGroupIndex, int(width), int(height)))


# ---- extensions ----------------------------------------------------------------------------------------
def GetTraceStats():
    st = _lib.rdx_trace_stats()
    _check(_lib.lib().rdx_get_trace_stats(C.byref(st)))
    return st


def GetVisitProfile(max_bounces=64):
    """(bounces, 2, 4) uint64: per bounce, per ray class (radiance, shadow): top nodes, instance visits,
    bottom nodes, triangle tests of the reference algorithm (after a frame traced with count_visits)"""
    out = np.zeros(8 * max_bounces, np.uint64)
    n = _lib.lib().rdx_get_visit_profile(out.ctypes.data, max_bounces)
    if n < 0:
        raise RadianceError(_lib.last_error())
    return out[:8 * n].reshape(n, 2, 4)


def GetBounceCounts(n=16):
    out = np.zeros(n, np.uint64)
    _check(_lib.lib().rdx_get_bounce_counts(out.ctypes.data, n))
    return out


def SetOption(name, value):
    _check(_lib.lib().rdx_set_option(name.encode(), int(value)))


def SetProfiling(on):
    _check(_lib.lib().rdx_set_profiling(1 if on else 0))


def SetShard(rank, world, tile_w=64, tile_h=64):
    _check(_lib.lib().rdx_set_shard(rank, world, tile_w, tile_h))


HIT_DTYPE = np.dtype([("hitPoint", "<f4", 3), ("distance", "<f4"), ("primitiveIndex", "<u4"), ("instanceIndex", "<u4"),
                      ("instanceCustomIndex", "<u4"), ("instanceSBTOffset", "<u4"), ("barycentric", "<f4", 3),
                      ("hit", "<u4"), ("transform", "<f4", 16)])
PAYLOAD_DTYPE = np.dtype([("color", "<f4", 3), ("hit", "<u4"), ("nextFactor", "<f4", 3),
                          ("nextRayOrigin", "<f4", 3), ("nextRayDirection", "<f4", 3)])
assert HIT_DTYPE.itemsize == C.sizeof(_lib.rdx_hit) and PAYLOAD_DTYPE.itemsize == C.sizeof(_lib.rdx_payload)


def TraceBatch(tlas, origins, dirs, tmin=0.001, tmax=1000.0, sbtRecordOffset=1, count_visits=False, reference_order=False):
    """Test seam: closest-hit (1) / any-hit (2) traversal of explicit rays -> structured array of HitData.
    Default = the production kernel; reference_order / count_visits use the reference-order kernel."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros(o.shape[0], HIT_DTYPE)
    visit = np.zeros(4, np.uint64)
    mode = 1 if (reference_order or count_visits) else 0
    _check(_lib.lib().rdx_trace_batch(tlas.handle, o.ctypes.data, d.ctypes.data, o.shape[0], tmin, tmax,
                                      sbtRecordOffset, mode, out.ctypes.data, visit.ctypes.data if count_visits else None))
    return (out, visit) if count_visits else out


# ---- the argument layer of the device-resident calls, QueryRays .. TraceAreaPathsTorch -----------------------
# Every call below has a Buffer route (device buffers in and out) and a torch route (CUDA tensors, wrapped and handed to the Buffer
# route).  What the two routes decide about their arguments is decided here once: the formats of the records, the rules of Buffer
# arguments and of created outputs, the integer checks, and the steps of a call on tensors.
_RECORDS = {}


def _record(kind, dtype, *torch_dtypes):
    """one row of the record table: a record kind's bytes, its torch columns (4-byte words; None: a one-dimensional tensor) and the
    names of the torch dtypes accepted for it, first the one a created tensor gets"""
    _RECORDS[kind] = (dtype.itemsize, dtype.itemsize // 4 if dtype.itemsize > 4 else None, torch_dtypes)


_record("float4", np.dtype(("<f4", 4)), "float32")       # lit, radiance, randoms, colours
_record("src", np.dtype("<u4"), "int32")
_record("pixel", np.dtype("<u4"), "int32")


def _buffers(who, **named):
    """the arguments of `who` that must be Buffers, by name"""
    if not all(isinstance(b, Buffer) for b in named.values()):
        *most, last = named
        if not most:
            raise RadianceError("%s: %s must be a Buffer (CreateBuffer / WrapDeviceMemory)" % (who, last))
        raise RadianceError("%s: %s and %s must be Buffers (CreateBuffer / WrapDeviceMemory)" % (who, ", ".join(most), last))


def _optional_buffer(who, buf, what):
    """-> the handle of an argument that is a Buffer or None"""
    if buf is not None and not isinstance(buf, Buffer):
        raise RadianceError("%s: %s must be a Buffer or None" % (who, what))
    return _h(buf)


def _h(buf):
    return buf.handle if buf is not None else None


def _out_buffer(who, n, buf, offset, kind, what, optional, or_true=None, flags=True):
    """an output argument: a Buffer; True, or None where it is not optional: created for n records of `kind` behind `offset`;
    None / False where it is optional: not wanted.  or_true: the refusal names True as a choice (default: where optional).
    flags=False: the position takes a Buffer or None alone, and True / False are refused like any other value"""
    if (buf is True and flags) or (buf is None and not optional):
        return CreateBuffer(None, max(int(offset) + _RECORDS[kind][0] * int(n), 1))
    if buf is None or (buf is False and flags):
        return None
    if not isinstance(buf, Buffer):
        raise RadianceError("%s: %s must be a Buffer%s" % (who, what, ", True or None" if (optional if or_true is None else or_true) else " or None"))
    return buf


def _is_count(x, most=None):
    """x is a non-negative integer, no bool, and at most `most`"""
    return not isinstance(x, bool) and isinstance(x, (int, np.integer)) and 0 <= x and (most is None or x <= most)


def _count(who, x, rule, most=None):
    """-> int(x), or the refusal `rule` in the words of the caller"""
    if not _is_count(x, most):
        raise RadianceError("%s: %s" % (who, rule))
    return int(x)


def _keys_or_randoms(who, keys, randoms):
    """-> the handles of `keys` and `randoms`, exactly one of which is a Buffer and the other None"""
    handles = _optional_buffer(who, keys, "keys"), _optional_buffer(who, randoms, "randoms")
    if keys is None and randoms is None:
        raise RadianceError("%s: neither keys nor randoms given: one of the two is required" % who)
    if keys is not None and randoms is not None:
        raise RadianceError("%s: both keys and randoms given: only one of the two is allowed" % who)
    return handles


def _cuda_tensor(who, t, kind, what, rows=None, device=None, owner="rays"):
    """-> the rows of `t`: a contiguous CUDA tensor of records of `kind`, of `rows` rows (None: any number), on `device` (the device
    of the owner's tensor) if one is given; anything else is a RadianceError"""
    import torch
    _, cols, names = _RECORDS[kind]
    shape = () if cols is None else (cols,)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and str(t.dtype).replace("torch.", "") in names and t.dim() == 1 + len(shape)
            and tuple(t.shape[1:]) == shape and rows in (None, t.shape[0]) and t.is_contiguous() and (device is None or t.device == device)):
        raise RadianceError("%s: %s must be a contiguous %s CUDA tensor of shape (n,%s)%s"
                            % (who, what, " / ".join(names), "" if cols is None else " %d" % cols, " on the %s' device" % owner if device is not None else ""))
    return int(t.shape[0])


class _TorchCall:
    """the torch route of one call.  `first` fixes n and the device; `also` holds a further tensor to them; `new` allocates an output;
    `begin` synchronises; `wrap` adopts a tensor as the Buffer the Buffer route takes"""

    def __init__(self, who):
        import torch
        self.torch, self.who, self.n, self.device = torch, who, None, None

    def first(self, t, kind, what, device=None, owner="rays"):
        self.n, self.device = _cuda_tensor(self.who, t, kind, what, None, device, owner), t.device

    def also(self, t, kind, what, owner="rays"):
        _cuda_tensor(self.who, t, kind, what, self.n, self.device, owner)

    def keys_or_randoms(self, keys, randoms):
        if (keys is None) == (randoms is None):
            raise RadianceError("%s: exactly one of keys and randoms must be given" % self.who)
        if keys is not None:
            self.also(keys, "key", "keys")
        if randoms is not None:
            self.also(randoms, "float4", "randoms")

    def new(self, kind, wanted=True):
        """an output tensor of n records of `kind`, or None where it is not wanted"""
        _, cols, names = _RECORDS[kind]
        if not wanted:
            return None
        shape = (self.n,) if cols is None else (self.n, cols)
        return self.torch.empty(shape, dtype=getattr(self.torch, names[0]), device=self.device)

    def given_or_new(self, t, kind, what):
        """an output tensor of the caller's, held to n and the device, or None: a new one"""
        if t is None:
            return self.new(kind)
        self.also(t, kind, what)
        return t

    def begin(self):
        """The library cannot see torch's stream, so the current stream is synchronised.  -> whether there is anything to do: with
        n == 0 nothing is wrapped and the library is not called"""
        self.torch.cuda.current_stream(self.device).synchronize()
        return self.n != 0

    def wrap(self, t, kind, rows=None):
        """the Buffer over the first `rows` (default: n) records of tensor `t`, which it keeps alive; None for None"""
        return WrapDeviceMemory(None, t.data_ptr(), (self.n if rows is None else rows) * _RECORDS[kind][0], keepalive=t) if t is not None else None


# ---- ray queries on device memory (rdx_query_rays) ---------------------------------------------------------------
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("hit", "<u4"), ("primitiveIndex", "<u4"),
                          ("instanceIndex", "<u4"), ("instanceCustomIndex", "<u4"), ("instanceSBTOffset", "<u4")])
assert RAY_DTYPE.itemsize == C.sizeof(_lib.rdx_ray) == 32 and RAY_HIT_DTYPE.itemsize == C.sizeof(_lib.rdx_ray_hit) == 32
_record("ray", RAY_DTYPE, "float32")
_record("hit", RAY_HIT_DTYPE, "int32", "float32")
QUERY_CLOSEST, QUERY_ANY = 1, 2


def QueryRays(tlas, rays, n, kind=QUERY_CLOSEST, hits=None, rays_offset=0, hits_offset=0):
    """Extension: `n` rays (RAY_DTYPE records, each with its own tmin / tmax) from the device buffer `rays` at byte `rays_offset`
    against `tlas`; one RAY_HIT_DTYPE record per ray goes to the device buffer `hits` at byte `hits_offset` (created when None:
    hits_offset + 32 n bytes).  kind: QUERY_CLOSEST (sbtRecordOffset 1) or QUERY_ANY (2: only `hit` is meaningful).  Nothing
    passes through the host.  Returns `hits`."""
    _buffers("QueryRays", tlas=tlas, rays=rays)
    hits = _out_buffer("QueryRays", n, hits, hits_offset, "hit", "hits", False, flags=False)
    _check(_lib.lib().rdx_query_rays(tlas.handle, rays.handle, int(rays_offset), int(n), int(kind), hits.handle, int(hits_offset)))
    return hits


def QueryRaysTorch(tlas, rays_tensor, kind=QUERY_CLOSEST, out=None):
    """Extension: rays from a contiguous float32 CUDA tensor of shape (n, 8) -- origin, tmin, direction, tmax per row; the records
    land in `out`, an int32 (or float32) CUDA tensor of shape (n, 8) (created when None: int32; `.view(torch.float32)` shows t,
    b1, b2).  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    t = _TorchCall("QueryRaysTorch")
    t.first(rays_tensor, "ray", "rays")
    out = t.given_or_new(out, "hit", "out")
    if t.begin():
        QueryRays(tlas, t.wrap(rays_tensor, "ray"), t.n, kind, t.wrap(out, "hit"))
    return out


# ---- surface records of a query's hits (rdx_resolve_hits) ----------------------------------------------------------
SURFACE_DTYPE = np.dtype([("position", "<f4", 3), ("hit", "<u4"), ("normal", "<f4", 3), ("materialIndex", "<u4"),
                          ("above", "<f4", 3), ("u", "<f4"), ("below", "<f4", 3), ("v", "<f4")])
assert SURFACE_DTYPE.itemsize == C.sizeof(_lib.rdx_surface) == 64
_record("surface", SURFACE_DTYPE, "float32")


class SurfaceBuffers:
    """rdx_surface_buffers: the Buffers bound to descriptor slots 5, 7, 8, 9; uv may be None (u = v = 0)"""

    def __init__(self, meshInfo, index, uv, normal):
        self.meshInfo, self.index, self.uv, self.normal = meshInfo, index, uv, normal

    def _struct(self):
        for name in ("meshInfo", "index", "normal"):
            if not isinstance(getattr(self, name), Buffer):
                raise RadianceError("ResolveHits: scene_buffers.%s must be a Buffer" % name)
        if self.uv is not None and not isinstance(self.uv, Buffer):
            raise RadianceError("ResolveHits: scene_buffers.uv must be a Buffer or None")
        return _lib.rdx_surface_buffers(self.meshInfo.handle, self.index.handle, self.uv.handle if self.uv is not None else None,
                                        self.normal.handle)


def ResolveHits(tlas, rays, hits, n, scene_buffers, out=None, rays_offset=0, hits_offset=0, out_offset=0):
    """Extension: one SURFACE_DTYPE record per ray -- world-space hit point, normal, the offset origins on either side of the
    surface, uv, material number -- for the `n` RAY_HIT_DTYPE records QueryRays(..., QUERY_CLOSEST) wrote to `hits` for `rays`;
    device buffers in, device buffer out (created when None: out_offset + 64 n bytes).  scene_buffers: a SurfaceBuffers, or a
    (meshInfo, index, uv, normal) tuple of Buffers.  Misses are 64 zero bytes; so are hits that would read outside a scene
    buffer, which are counted.  Returns (out, invalid)."""
    _buffers("ResolveHits", tlas=tlas, rays=rays, hits=hits)
    if not isinstance(scene_buffers, SurfaceBuffers):
        try:
            scene_buffers = SurfaceBuffers(*scene_buffers)
        except TypeError:
            raise RadianceError("ResolveHits: scene_buffers must be a SurfaceBuffers or a (meshInfo, index, uv, normal) tuple")
    sb = scene_buffers._struct()
    out = _out_buffer("ResolveHits", n, out, out_offset, "surface", "out", False, flags=False)
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_resolve_hits(tlas.handle, rays.handle, int(rays_offset), hits.handle, int(hits_offset), int(n), C.byref(sb),
                                       out.handle, int(out_offset), C.byref(invalid)))
    return out, int(invalid.value)


def ResolveHitsTorch(tlas, rays_tensor, hits_tensor, scene_buffers, out=None):
    """Extension: ResolveHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32 (n, 8)
    tensor QueryRaysTorch returned for them; the records land in `out`, a contiguous float32 CUDA tensor of shape (n, 16)
    (created when None; `.view(torch.int32)` shows hit and materialIndex in columns 3 and 7).  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks.  Returns (out, invalid)."""
    t = _TorchCall("ResolveHitsTorch")
    t.first(rays_tensor, "ray", "rays")
    t.also(hits_tensor, "hit", "hits")
    out = t.given_or_new(out, "surface", "out")
    invalid = 0
    if t.begin():
        _, invalid = ResolveHits(tlas, t.wrap(rays_tensor, "ray"), t.wrap(hits_tensor, "hit"), t.n, scene_buffers, t.wrap(out, "surface"))
    return out, invalid


def DebugSurfaceInBounds(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, nmeshinfo=None):
    """Test seam (rdx_debug_surface_in_bounds): the bounds rule of ResolveHits for one record, on the host -> bool.  meshInfo: a
    MeshInfo array (nmeshinfo defaults to its length), idx3: the triangle's three vertex numbers or None."""
    shared = _bounds_arguments(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, nmeshinfo)
    return _in_bounds(_lib.lib().rdx_debug_surface_in_bounds(*shared))


def _bounds_arguments(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, nmeshinfo):
    """what DebugSurfaceInBounds and DebugShadeInBounds hand to the library alike, in its order (the pointer keeps its array alive)"""
    mi = np.ascontiguousarray(meshInfo, MeshInfo).reshape(-1)
    iv = None if idx3 is None else (C.c_uint32 * 3)(*[int(x) & 0xffffffff for x in idx3])
    nm = mi.shape[0] if nmeshinfo is None else int(nmeshinfo)
    return (mi.ctypes.data_as(C.POINTER(_lib.rdx_mesh_info)), int(ninst), nm, int(instanceIndex) & 0xffffffff, int(primitiveIndex) & 0xffffffff, iv,
            int(nindex), int(nnormal), int(nuv))


def _in_bounds(rc):
    if rc < 0:
        raise RadianceError(_lib.last_error())
    return rc == 1


def DebugCheckRanges(rows, first_out, n):
    """Test seam (rdx_debug_check_ranges): the range rule of every device-resident call from QueryRays to TraceLightPaths, on plain
    numbers, on the host.  rows: (name, address, size, offset, bytes, align, present) per range, inputs first; rows from
    `first_out` on are outputs.  Returns None if the call would be accepted, else the refusal's text."""
    rows = list(rows)
    R = (_lib.rdx_debug_range * max(len(rows), 1))()
    for k, (_, address, size, offset, nbytes, align, present) in enumerate(rows):
        R[k] = _lib.rdx_debug_range(int(address), int(size), int(offset), int(nbytes), int(align), 1 if present else 0)
    names = (C.c_char_p * max(len(rows), 1))(*[str(r[0]).encode() for r in rows])
    rc = _lib.lib().rdx_debug_check_ranges(R, names, len(rows), int(first_out), int(n))
    return None if rc == 0 else _lib.last_error()


# ---- the stock closest-hit shader on a query's hits (rdx_shade_hits) --------------------------------------------------
SHADE_KEY_DTYPE = np.dtype([("frameID", "<u4"), ("pixel", "<u4"), ("depth", "<u4"), ("_0", "<u4")])
SHADE_DTYPE = np.dtype([("color", "<f4", 3), ("hit", "<u4"), ("colorOccluded", "<f4", 3), ("materialIndex", "<u4"),
                        ("nextFactor", "<f4", 3), ("slot", "<u4")])
assert SHADE_DTYPE.itemsize == C.sizeof(_lib.rdx_shade) == 48 and SHADE_KEY_DTYPE.itemsize == C.sizeof(_lib.rdx_shade_key) == 16
assert C.sizeof(_lib.rdx_shading_buffers) == 8 * C.sizeof(C.c_void_p)
_record("key", SHADE_KEY_DTYPE, "int32")
_record("shade", SHADE_DTYPE, "float32")
NO_SLOT = 0xffffffff


class ShadingBuffers:
    """rdx_shading_buffers: the Buffers bound to descriptor slots 4, 5, 7, 8, 9, 10, the image array of slot 11 and the Sampler of
    slot 12; uv, textureArray and sampler may be None"""
    _REQUIRED = ("scene", "meshInfo", "index", "normal", "material")

    def __init__(self, scene, meshInfo, index, uv, normal, material, textureArray=None, sampler=None):
        self.scene, self.meshInfo, self.index, self.uv, self.normal, self.material = scene, meshInfo, index, uv, normal, material
        self.textureArray, self.sampler = textureArray, sampler

    def _struct(self, who="ShadeHits"):
        for name in self._REQUIRED:
            if not isinstance(getattr(self, name), Buffer):
                raise RadianceError("%s: scene_buffers.%s must be a Buffer" % (who, name))
        for name in ("uv", "textureArray"):
            if getattr(self, name) is not None and not isinstance(getattr(self, name), Buffer):
                raise RadianceError("%s: scene_buffers.%s must be a Buffer or None" % (who, name))
        if self.sampler is not None and not isinstance(self.sampler, Sampler):
            raise RadianceError("%s: scene_buffers.sampler must be a Sampler or None" % who)
        return _lib.rdx_shading_buffers(self.scene.handle, self.meshInfo.handle, self.index.handle, _h(self.uv), self.normal.handle,
                                        self.material.handle, _h(self.textureArray), _h(self.sampler))


def _shading_struct(who, scene_buffers):
    """the rdx_shading_buffers of a ShadingBuffers, or of a tuple of its constructor's arguments"""
    if not isinstance(scene_buffers, ShadingBuffers):
        try:
            scene_buffers = ShadingBuffers(*scene_buffers)
        except TypeError:
            raise RadianceError("%s: scene_buffers must be a ShadingBuffers or a (scene, meshInfo, index, uv, normal, material"
                                "[, textureArray, sampler]) tuple" % who)
    return scene_buffers._struct(who)


def ShadeHits(tlas, rays, hits, keys, n, scene_buffers, shade=None, next=True, shadow=True, src=None, compact=False, rays_offset=0,
              hits_offset=0, keys_offset=0, shade_offset=0, next_offset=0, shadow_offset=0, src_offset=0):
    """Extension: the stock closest-hit / miss shaders on the `n` RAY_HIT_DTYPE records QueryRays(..., QUERY_CLOSEST) wrote to `hits`
    for `rays`, with the SHADE_KEY_DTYPE records of `keys` as the RNG inputs (frameID, pixel, depth); device buffers in, device
    buffers out.  scene_buffers: a ShadingBuffers or a tuple of its constructor's arguments.  One SHADE_DTYPE record per ray goes
    to `shade`: `color` if the ray's shadow ray is not occluded, `colorOccluded` if it is, `nextFactor`, and `slot` = the record
    number k of the ray's next ray in `next` and of its shadow ray in `shadow` (RAY_DTYPE records, ready for QueryRays), NO_SLOT
    for a ray that does not survive.  shade: a Buffer, or None (created).  next / shadow: a Buffer, True (created: n records) or
    None / False (not wanted; without `next` the next direction is not sampled).  src: a Buffer, or None -- then compact=True
    creates it.  With `src`, the survivors are packed into records 0 .. live - 1 (those of 64 consecutive input rays contiguous and
    in input order, the groups in no fixed order), src[k] = the ray's number, and records from `live` on are untouched; without,
    k = i and the record of a ray that does not survive is zeros.  Returns (shade, next, shadow, src, live, invalid): `live`
    survivors; `invalid` hits that would read outside a scene buffer, zeroed and counted."""
    _buffers("ShadeHits", tlas=tlas, rays=rays, hits=hits, keys=keys)
    sb = _shading_struct("ShadeHits", scene_buffers)
    n = int(n)
    shade = _out_buffer("ShadeHits", n, shade, shade_offset, "shade", "shade", False)
    next = _out_buffer("ShadeHits", n, next, next_offset, "ray", "next", True)
    shadow = _out_buffer("ShadeHits", n, shadow, shadow_offset, "ray", "shadow", True)
    src = _out_buffer("ShadeHits", n, True if (src is None and compact) else src, src_offset, "src", "src", True)
    live, invalid = C.c_uint32(0), C.c_uint32(0)
    _check(_lib.lib().rdx_shade_hits(tlas.handle, rays.handle, int(rays_offset), hits.handle, int(hits_offset), keys.handle, int(keys_offset), n,
                                     C.byref(sb), shade.handle, int(shade_offset), _h(next), int(next_offset), _h(shadow), int(shadow_offset),
                                     _h(src), int(src_offset), C.byref(live), C.byref(invalid)))
    return shade, next, shadow, src, int(live.value), int(invalid.value)


def ShadeHitsTorch(tlas, rays_t, hits_t, keys_t, scene_buffers, compact=True, sample_next=True):
    """Extension: ShadeHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32 (n, 8)
    tensor QueryRaysTorch returned for them, keys a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0).  Returns (shade,
    next, shadow, src, live, invalid): shade float32 (n, 12) (`.view(torch.int32)` shows hit, materialIndex and slot in columns 3,
    7, 11), next / shadow float32 (live, 8) when compacting -- already sliced to the survivors -- else (n, 8), src int32 (live,)
    or None; next is None without sample_next.  The library cannot see torch's stream, so the current stream is synchronised
    first; the call blocks."""
    t = _TorchCall("ShadeHitsTorch")
    t.first(rays_t, "ray", "rays")
    t.also(hits_t, "hit", "hits")
    t.also(keys_t, "key", "keys")
    shade = t.new("shade")
    nxt = t.new("ray", sample_next)
    shadow = t.new("ray")
    src = t.new("src", compact)
    live = invalid = 0
    if t.begin():
        _, _, _, _, live, invalid = ShadeHits(tlas, t.wrap(rays_t, "ray"), t.wrap(hits_t, "hit"), t.wrap(keys_t, "key"), t.n, scene_buffers,
                                              t.wrap(shade, "shade"), t.wrap(nxt, "ray"), t.wrap(shadow, "ray"), t.wrap(src, "src"))
    if compact:
        nxt, shadow, src = (nxt[:live] if nxt is not None else None), shadow[:live], src[:live]
    return shade, nxt, shadow, src, live, invalid


def DebugShadeInBounds(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, materials, textures=False, layers=0,
                       nmeshinfo=None, nmaterials=None):
    """Test seam (rdx_debug_shade_in_bounds): the bounds rule of ShadeHits for one record, on the host -> bool.  As
    DebugSurfaceInBounds, plus `materials`: a Material array (nmaterials defaults to its length), textures: texels are read,
    layers: layers of the image array."""
    mt = np.ascontiguousarray(materials, Material).reshape(-1)
    nmat = mt.shape[0] if nmaterials is None else int(nmaterials)
    shared = _bounds_arguments(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, nmeshinfo)
    rc = _lib.lib().rdx_debug_shade_in_bounds(*shared, mt.ctypes.data_as(C.POINTER(_lib.rdx_material)), nmat, 1 if textures else 0, int(layers))
    return _in_bounds(rc)


# ---- the evaluated material of a query's hits, and one light's direct term (rdx_resolve_materials, rdx_light_hits) --------
MATERIAL_RECORD_DTYPE = np.dtype([("normal", "<f4", 3), ("hit", "<u4"), ("albedo", "<f4", 3), ("materialIndex", "<u4"), ("metallic", "<f4"),
                                  ("roughness", "<f4"), ("transmission", "<f4"), ("ior", "<f4"), ("above", "<f4", 3), ("_0", "<u4")])
assert MATERIAL_RECORD_DTYPE.itemsize == C.sizeof(_lib.rdx_material_record) == 64
_record("material", MATERIAL_RECORD_DTYPE, "float32")
MAX_LIGHTS = 5          # the DirLights of a SceneProperties


def ResolveMaterials(tlas, rays, hits, n, scene_buffers, out=None, rays_offset=0, hits_offset=0, out_offset=0):
    """Extension: one MATERIAL_RECORD_DTYPE record per ray -- the shading normal (normal map applied), the sampled albedo, metallic,
    roughness, transmission, ior, the shadow ray's origin `above` and the material number, as the stock closest-hit shader holds
    them -- for the `n` RAY_HIT_DTYPE records QueryRays(..., QUERY_CLOSEST) wrote to `hits` for `rays`; device buffers in, device
    buffer out (created when None: out_offset + 64 n bytes).  scene_buffers: a ShadingBuffers or a tuple of its constructor's
    arguments, textures by ShadeHits' rule.  Misses are 64 zero bytes; so are hits that would read outside a scene buffer, which
    are counted.  Returns (out, invalid)."""
    _buffers("ResolveMaterials", tlas=tlas, rays=rays, hits=hits)
    sb = _shading_struct("ResolveMaterials", scene_buffers)
    out = _out_buffer("ResolveMaterials", n, out, out_offset, "material", "out", False, flags=False)
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_resolve_materials(tlas.handle, rays.handle, int(rays_offset), hits.handle, int(hits_offset), int(n), C.byref(sb),
                                            out.handle, int(out_offset), C.byref(invalid)))
    return out, int(invalid.value)


def LightHits(rays, materials, n, scene, light, lit=None, shadow=True, rays_offset=0, materials_offset=0, lit_offset=0, shadow_offset=0):
    """Extension: the direct term of directional light `light` (0 .. 4) of the SceneProperties in the device buffer `scene`
    (descriptor slot 4) for the `n` MATERIAL_RECORD_DTYPE records of `materials` (ResolveMaterials', or the caller's own) and the
    directions of `rays`: one float4 (rgb, 0) per ray goes to `lit` (a Buffer, or None: created), and the shadow ray towards the
    light, a RAY_DTYPE record ready for QueryRays(..., QUERY_ANY), to `shadow` (a Buffer, True: created, None / False: not wanted).
    Records whose `hit` is not 1 give zeros.  The ambient term (albedo * 0.1 in the stock shader) stays the caller's.  Returns
    (lit, shadow)."""
    _buffers("LightHits", rays=rays, materials=materials, scene=scene)
    n, light = int(n), _scene_light("LightHits", light)
    lit, shadow = _lit_and_shadow("LightHits", n, lit, lit_offset, shadow, shadow_offset)
    _check(_lib.lib().rdx_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, scene.handle, light, lit.handle,
                                     int(lit_offset), _h(shadow), int(shadow_offset)))
    return lit, shadow


def _scene_light(who, light):
    light = int(light)
    if not 0 <= light < MAX_LIGHTS:
        raise RadianceError("%s: light %d is not one of the %d lights of a SceneProperties (0 .. %d)" % (who, light, MAX_LIGHTS, MAX_LIGHTS - 1))
    return light


def _lit_and_shadow(who, n, lit, lit_offset, shadow, shadow_offset):
    """the outputs of the three per-light calls: lit, a Buffer or None (created); shadow, a Buffer, True (created) or None / False"""
    lit = _out_buffer(who, n, lit, lit_offset, "float4", "lit", False, flags=False)
    shadow = _out_buffer(who, n, shadow, shadow_offset, "ray", "shadow", True)
    return lit, shadow


def ResolveMaterialsTorch(tlas, rays_tensor, hits_tensor, scene_buffers, out=None):
    """Extension: ResolveMaterials on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32
    (n, 8) tensor QueryRaysTorch returned for them; the records land in `out`, a contiguous float32 CUDA tensor of shape (n, 16)
    (created when None): columns 0-2 the normal, 4-6 the albedo, 8-11 metallic, roughness, transmission, ior, 12-14 `above`;
    `.view(torch.int32)` shows hit and materialIndex in columns 3 and 7.  The library cannot see torch's stream, so the current
    stream is synchronised first; the call blocks.  Returns (out, invalid)."""
    t = _TorchCall("ResolveMaterialsTorch")
    t.first(rays_tensor, "ray", "rays")
    t.also(hits_tensor, "hit", "hits")
    out = t.given_or_new(out, "material", "out")
    invalid = 0
    if t.begin():
        _, invalid = ResolveMaterials(tlas, t.wrap(rays_tensor, "ray"), t.wrap(hits_tensor, "hit"), t.n, scene_buffers, t.wrap(out, "material"))
    return out, invalid


def LightHitsTorch(rays_t, materials_t, scene_buffer, light, want_shadow=True):
    """Extension: LightHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, materials the contiguous float32 (n, 16)
    tensor ResolveMaterialsTorch returned for them (or the caller's own records), scene_buffer the Buffer of descriptor slot 4.
    Returns (lit, shadow): lit float32 (n, 4) (rgb, 0), shadow float32 (n, 8) -- the rays QueryRaysTorch(..., QUERY_ANY) takes --
    or None without want_shadow.  The library cannot see torch's stream, so the current stream is synchronised first; the call
    blocks."""
    t = _TorchCall("LightHitsTorch")
    t.first(rays_t, "ray", "rays")
    t.also(materials_t, "material", "materials")
    if not isinstance(scene_buffer, Buffer):
        raise RadianceError("LightHitsTorch: scene_buffer must be a Buffer (the SceneProperties of descriptor slot 4)")
    light = _scene_light("LightHitsTorch", light)
    lit, shadow = t.new("float4"), t.new("ray", want_shadow)
    if t.begin():
        LightHits(t.wrap(rays_t, "ray"), t.wrap(materials_t, "material"), t.n, scene_buffer, light, t.wrap(lit, "float4"), t.wrap(shadow, "ray"))
    return lit, shadow


# ---- the next ray of a query's hits from material and surface records (rdx_scatter_hits) --------------------------------
SCATTER_DTYPE = np.dtype([("nextFactor", "<f4", 3), ("slot", "<u4")])
assert SCATTER_DTYPE.itemsize == C.sizeof(_lib.rdx_scatter) == 16
_record("scatter", SCATTER_DTYPE, "float32")


def ScatterHits(rays, materials, surfaces, keys, n, randoms=None, scatter=None, next=None, src=None, compact=False, rays_offset=0,
                materials_offset=0, surfaces_offset=0, keys_offset=0, randoms_offset=0, scatter_offset=0, next_offset=0, src_offset=0):
    """Extension: the next ray of the `n` MATERIAL_RECORD_DTYPE records of `materials` (ResolveMaterials', or the caller's own), the
    SURFACE_DTYPE records of `surfaces` (ResolveHits': only `below` is read) and the directions of `rays` -- the stock closest-hit
    shader's next-direction sample, nextFactor and choice of the offset origin.  The random numbers are pcg3d of the
    SHADE_KEY_DTYPE records of `keys` (frameID, pixel, depth), or -- keys None -- the float4 records of `randoms` (xyz as they
    are, w ignored): exactly one of the two is given.  One SCATTER_DTYPE record per ray goes to `scatter`: `nextFactor`, and
    `slot` = the record number k of the ray's next ray in `next` (RAY_DTYPE records, ready for QueryRays), NO_SLOT for a record
    whose `hit` is not 1.  scatter / next: a Buffer, or None (created).  src: a Buffer, or None -- then compact=True creates it.
    With `src`, the survivors are packed into records 0 .. live - 1 (those of 64 consecutive input rays contiguous and in input
    order, the groups in no fixed order), src[k] = the ray's number, and records from `live` on are untouched; without, k = i
    and the record of a ray that does not survive is zeros.  Returns (scatter, next, src, live)."""
    _buffers("ScatterHits", rays=rays, materials=materials, surfaces=surfaces)
    hk, hr = _keys_or_randoms("ScatterHits", keys, randoms)
    n = int(n)
    scatter = _out_buffer("ScatterHits", n, scatter, scatter_offset, "scatter", "scatter", False)
    next = _out_buffer("ScatterHits", n, next, next_offset, "ray", "next", False)
    src = _out_buffer("ScatterHits", n, True if (src is None and compact) else src, src_offset, "src", "src", True, or_true=False)
    live = C.c_uint32(0)
    _check(_lib.lib().rdx_scatter_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), surfaces.handle, int(surfaces_offset),
                                       hk, int(keys_offset), hr, int(randoms_offset), n, scatter.handle, int(scatter_offset),
                                       next.handle, int(next_offset), _h(src), int(src_offset), C.byref(live)))
    return scatter, next, src, int(live.value)


def ScatterHitsTorch(rays_t, materials_t, surfaces_t, keys_t=None, randoms_t=None, compact=True):
    """Extension: ScatterHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, materials / surfaces the contiguous float32
    (n, 16) tensors ResolveMaterialsTorch / ResolveHitsTorch returned for them (or the caller's own records), and exactly one of
    keys, a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0), and randoms, a contiguous float32 (n, 4) tensor (xyz used).
    Returns (scatter, next, src, live): scatter float32 (n, 4) (nextFactor; `.view(torch.int32)` shows slot in column 3), next
    float32 (live, 8) when compacting -- already sliced to the survivors -- else (n, 8), src int32 (live,) or None.  The library
    cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    t = _TorchCall("ScatterHitsTorch")
    t.first(rays_t, "ray", "rays")
    t.also(materials_t, "material", "materials")
    t.also(surfaces_t, "surface", "surfaces")
    t.keys_or_randoms(keys_t, randoms_t)
    scatter = t.new("scatter")
    nxt = t.new("ray")
    src = t.new("src", compact)
    live = 0
    if t.begin():
        _, _, _, live = ScatterHits(t.wrap(rays_t, "ray"), t.wrap(materials_t, "material"), t.wrap(surfaces_t, "surface"), t.wrap(keys_t, "key"), t.n,
                                    t.wrap(randoms_t, "float4"), t.wrap(scatter, "scatter"), t.wrap(nxt, "ray"), t.wrap(src, "src"))
    if compact:
        nxt, src = nxt[:live], src[:live]
    return scatter, nxt, src, live


# ---- the two ends of a frame on device memory (rdx_generate_rays, rdx_accumulate) ---------------------------------------
RAYGEN_SEED_DTYPE = np.dtype([("in", "<u4", 3), ("_0", "<u4")])
assert RAYGEN_SEED_DTYPE.itemsize == C.sizeof(_lib.rdx_raygen_seed) == 16
_record("seed", RAYGEN_SEED_DTYPE, "int32")
ACCUMULATE_DEBUG = 1


def GenerateRays(camera, n, frame_id, total_samples, first_pixel=0, pixels=None, seeds=None, tmin=0.001, tmax=1000.0, rays=None, keys=True,
                 pixels_offset=0, seeds_offset=0, rays_offset=0, keys_offset=0):
    """Extension: `n` camera rays of the PhysicalCamera in the device buffer `camera` (the contents of descriptor slot 3; it need
    not be bound, and is read on the device by every call), as RAY_DTYPE records in `rays` -- ready for QueryRays -- and
    SHADE_KEY_DTYPE records (frame_id, pixel, 0, 0) in `keys` -- the keys of depth 0 for ShadeHits.  Ray i belongs to pixel
    first_pixel + i, or pixels[i] (`pixels`: a Buffer of uint32); its random input is pcg3d(frame_id, total_samples, pixel) as in
    the reference's raygen, or pcg3d of seeds[i] (`seeds`: a Buffer of RAYGEN_SEED_DTYPE).  Every ray has the bits of the frame
    path's generateRay; tmin / tmax are written as given.  rays: a Buffer, or None (created).  keys: a Buffer, True (created) or
    None / False (not wanted).  Nothing passes through the host.  Returns (rays, keys)."""
    _buffers("GenerateRays", camera=camera)
    n = int(n)
    rays = _out_buffer("GenerateRays", n, rays, rays_offset, "ray", "rays", False, flags=False)
    hp, hs = _optional_buffer("GenerateRays", pixels, "pixels"), _optional_buffer("GenerateRays", seeds, "seeds")
    keys = _out_buffer("GenerateRays", n, keys, keys_offset, "key", "keys", True, or_true=False)
    _check(_lib.lib().rdx_generate_rays(camera.handle, n, int(first_pixel), hp, int(pixels_offset), int(frame_id), int(total_samples), hs,
                                        int(seeds_offset), float(tmin), float(tmax), rays.handle, int(rays_offset), _h(keys), int(keys_offset)))
    return rays, keys


def GenerateRaysTorch(camera, n_or_pixels, frame_id, total_samples, seeds=None):
    """Extension: GenerateRays into CUDA tensors.  n_or_pixels: an int n (pixels 0 .. n - 1), or a contiguous int32 CUDA tensor of
    pixel numbers, shape (n,).  seeds: None, or a contiguous int32 CUDA tensor of shape (n, 4) (the three inputs of pcg3d, 0).
    Returns (rays float32 (n, 8): origin, tmin = 0.001, direction, tmax = 1000 per row -- what QueryRaysTorch takes; keys int32
    (n, 4): frame_id, pixel, 0, 0 -- what ShadeHitsTorch takes at depth 0).  The library cannot see torch's stream, so the
    current stream is synchronised first; the call blocks."""
    t = _TorchCall("GenerateRaysTorch")
    px = None
    if isinstance(n_or_pixels, t.torch.Tensor):
        px = n_or_pixels
        t.first(px, "pixel", "pixels")
    elif _is_count(n_or_pixels):
        t.n, t.device = int(n_or_pixels), t.torch.device("cuda", t.torch.cuda.current_device())
    else:
        raise RadianceError("GenerateRaysTorch: the second argument is a ray count or an int32 CUDA tensor of pixel numbers")
    if seeds is not None:
        t.also(seeds, "seed", "seeds", owner="pixels")
    rays, keys = t.new("ray"), t.new("key")
    if t.begin():
        GenerateRays(camera, t.n, frame_id, total_samples, 0, t.wrap(px, "pixel"), t.wrap(seeds, "seed"), rays=t.wrap(rays, "ray"), keys=t.wrap(keys, "key"))
    return rays, keys


def Accumulate(colors, n, frame_id, scratch, image=None, first_pixel=0, pixels=None, debug=False, colors_offset=0, pixels_offset=0):
    """Extension: the end of a frame's sample on the device.  colors: a Buffer of `n` float4 records (rgb, w ignored), sample
    `frame_id` of pixels first_pixel + i, or pixels[i] (`pixels`: a Buffer of uint32).  scratch (imageScratch, float4 per pixel)
    takes the reference's running mean -- rgb = colour for frame_id 0, else (frame_id * rgb + colour) / (frame_id + 1) in
    float32, w kept -- and image (RGBA8, optional) the tone-mapped mean of those pixels (debug: no ACES, no gamma).  One call is
    one frame_id; its pixels must be distinct (of two samples of one pixel one wins, unspecified which).  Returns `invalid`:
    the samples whose pixel number is not below min(scratch.size / 16, image.size / 4); they write nothing."""
    _buffers("Accumulate", colors=colors, scratch=scratch)
    hi, hp = _optional_buffer("Accumulate", image, "image"), _optional_buffer("Accumulate", pixels, "pixels")
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_accumulate(colors.handle, int(colors_offset), int(n), int(first_pixel), hp, int(pixels_offset), int(frame_id),
                                     scratch.handle, hi, ACCUMULATE_DEBUG if debug else 0, C.byref(invalid)))
    return int(invalid.value)


def AccumulateTorch(colors, frame_id, scratch, image=None, pixels=None, debug=False):
    """Extension: Accumulate on CUDA tensors.  colors: contiguous float32 (n, 4); pixels: None (pixels 0 .. n - 1) or a contiguous
    int32 (n,) tensor; scratch / image: Buffers (e.g. a DeviceScene's rdImageScratch / rdImage), or contiguous tensors of shape
    (npix, 4), float32 / uint8, which are updated in place.  Returns `invalid`.  The library cannot see torch's stream, so the
    current stream is synchronised first; the call blocks."""
    t = _TorchCall("AccumulateTorch")
    torch = t.torch
    t.first(colors, "float4", "colors")
    if pixels is not None:
        t.also(pixels, "pixel", "pixels", owner="colours")

    def frame(f, dtype, what):
        if f is None or isinstance(f, Buffer):
            return f
        if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == dtype and f.dim() == 2 and f.shape[1] == 4 and f.is_contiguous()
                and f.device == t.device):
            raise RadianceError("AccumulateTorch: %s must be a Buffer or a contiguous %s CUDA tensor of shape (npix, 4) on the colours' device"
                                % (what, str(dtype).replace("torch.", "")))
        return WrapDeviceMemory(None, f.data_ptr(), f.numel() * f.element_size(), keepalive=f) if f.numel() else None
    if scratch is None:
        raise RadianceError("AccumulateTorch: scratch must be a Buffer or a float32 CUDA tensor of shape (npix, 4)")
    bs, bi = frame(scratch, torch.float32, "scratch"), frame(image, torch.uint8, "image")
    if not t.begin():
        return 0
    if bs is None or (image is not None and bi is None):       # a frame of no pixels: every sample is outside it
        return t.n
    return Accumulate(t.wrap(colors, "float4"), t.n, frame_id, bs, bi, 0, t.wrap(pixels, "pixel"), debug)


# ---- radiance along the caller's own rays (rdx_trace_paths) -------------------------------------------------------------
def _path_arguments(who, n, max_depth, scene_buffers, **buffers):
    """the preamble of the four path calls, in the order of its refusals: the Buffers (tlas, rays, keys and the call's own),
    scene_buffers, n and max_depth -> the rdx_shading_buffers and int(n).  The path calls type-check n; the per-hit calls coerce it"""
    _buffers(who, **buffers)
    sb = _shading_struct(who, scene_buffers)
    if not (_is_count(n) and _is_count(max_depth)):
        raise RadianceError("%s: n and max_depth must be non-negative integers" % who)
    return sb, int(n)


def TracePaths(tlas, rays, keys, n, max_depth, scene_buffers, radiance=None, hits=None, rays_offset=0, keys_offset=0, radiance_offset=0,
               hits_offset=0):
    """Extension: the reference's raygen loop for `n` rays of the caller's own, on the frame path's stages.  Path i starts with the
    RAY_DTYPE record i of `rays` (its own tmin / tmax for the first segment; 0.001 / 1000 after it) and the SHADE_KEY_DTYPE
    record i of `keys` (frameID, pixel; depth and _0 are ignored) and is followed for at most `max_depth` (0 .. 62) segments;
    one float4 (rgb, 0) per path goes to `radiance`: the bits of the loop over QueryRays / ShadeHits, the sample Accumulate
    expects.  scene_buffers: a ShadingBuffers or a tuple of its constructor's arguments; it must describe the scene of `tlas` (the
    shade stage gathers unchecked, as TraceRays does).  radiance: a Buffer, or None (created: radiance_offset + 16 n bytes).
    hits: a Buffer, True (created) or None / False (not wanted): the RAY_HIT_DTYPE records of the first segment, as
    QueryRays(..., QUERY_CLOSEST) writes them.  Device buffers in and out; nothing passes through the host.  Returns `radiance`
    (the hit buffer is `hits` where the caller passed one; rd.TracePaths(..., hits=True) returns (radiance, hits))."""
    sb, n = _path_arguments("TracePaths", n, max_depth, scene_buffers, tlas=tlas, rays=rays, keys=keys)
    radiance = _out_buffer("TracePaths", n, radiance, radiance_offset, "float4", "radiance", False, flags=False)
    made_hits = hits is True
    hits = _out_buffer("TracePaths", n, hits, hits_offset, "hit", "hits", True, or_true=False)
    _check(_lib.lib().rdx_trace_paths(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), C.byref(sb),
                                      radiance.handle, int(radiance_offset), _h(hits), int(hits_offset)))
    return (radiance, hits) if made_hits else radiance


def TracePathsTorch(tlas, rays_t, keys_t, max_depth, scene_buffers, want_hits=False):
    """Extension: TracePaths on CUDA tensors -- rays a contiguous float32 (n, 8) tensor (origin, tmin, direction, tmax per row), keys
    a contiguous int32 (n, 4) tensor (frameID, pixel, -, -): what GenerateRaysTorch returns, or rays of the caller's own.
    Returns radiance float32 (n, 4): rgb, 0 -- what AccumulateTorch takes -- and, with want_hits, (radiance, hits int32 (n, 8)).
    The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    t = _TorchCall("TracePathsTorch")
    t.first(rays_t, "ray", "rays")
    t.also(keys_t, "key", "keys")
    _count("TracePathsTorch", max_depth, "max_depth must be a non-negative integer")
    radiance, hits = t.new("float4"), t.new("hit", want_hits)
    if t.begin():
        TracePaths(tlas, t.wrap(rays_t, "ray"), t.wrap(keys_t, "key"), t.n, max_depth, scene_buffers, t.wrap(radiance, "float4"), t.wrap(hits, "hit"))
    return (radiance, hits) if want_hits else radiance


# ---- radiance along the caller's own rays, every light of the scene sampled (rdx_trace_paths_lights) ---------------------
def _light_count(who, light_count):
    return _count(who, light_count, "light_count must be an integer from 0 to 5 (the lights of a SceneProperties)", 5)


def TraceLightPaths(tlas, rays, keys, n, max_depth, light_count, scene_buffers, radiance=None, rays_offset=0, keys_offset=0, radiance_offset=0):
    """Extension: TracePaths with the first `light_count` (0 .. 5) directional lights of scene_buffers.scene sampled at every hit --
    the path tracer over QueryRays / ResolveHits / ResolveMaterials / LightHits / ScatterHits (the README's second loop) in one
    call, with its bits.  Rays and keys as for TracePaths.  The lights are read on the device by every call.  The call gathers
    checked: a hit that scene_buffers does not describe is a miss and is counted.  radiance: a Buffer, or None (created:
    radiance_offset + 16 n bytes).  Device buffers in and out.  Returns (radiance, invalid)."""
    sb, n = _path_arguments("TraceLightPaths", n, max_depth, scene_buffers, tlas=tlas, rays=rays, keys=keys)
    light_count = _light_count("TraceLightPaths", light_count)
    radiance = _out_buffer("TraceLightPaths", n, radiance, radiance_offset, "float4", "radiance", False, flags=False)
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_trace_paths_lights(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), light_count,
                                             C.byref(sb), radiance.handle, int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TraceLightPathsTorch(tlas, rays_t, keys_t, max_depth, light_count, scene_buffers):
    """Extension: TraceLightPaths on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, keys a contiguous int32 (n, 4) tensor, as
    for TracePathsTorch.  Returns radiance float32 (n, 4): rgb, 0 -- what AccumulateTorch takes.  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks."""
    t = _TorchCall("TraceLightPathsTorch")
    t.first(rays_t, "ray", "rays")
    t.also(keys_t, "key", "keys")
    _count("TraceLightPathsTorch", max_depth, "max_depth must be a non-negative integer")
    light_count = _light_count("TraceLightPathsTorch", light_count)
    radiance = t.new("float4")
    if t.begin():
        TraceLightPaths(tlas, t.wrap(rays_t, "ray"), t.wrap(keys_t, "key"), t.n, max_depth, light_count, scene_buffers, t.wrap(radiance, "float4"))
    return radiance


# ---- point and spot lights from a caller's light table (rdx_punctual_light_hits, rdx_trace_paths_punctual) -----------------
PUNCTUAL_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("type", "<u4"), ("direction", "<f4", 3), ("range", "<f4"), ("color", "<f4", 3),
                                 ("_0", "<f4"), ("coneScale", "<f4"), ("coneOffset", "<f4"), ("_1", "<f4"), ("_2", "<f4")])
assert PUNCTUAL_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_punctual_light) == 64
_record("light", PUNCTUAL_LIGHT_DTYPE, "float32")
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2
MAX_PATH_LIGHTS = 16     # the records of a table one TracePunctualPaths call samples


def SpotCone(inner_rad, outer_rad):
    """(coneScale, coneOffset) of a spot record as float32, for the cone's inner and outer half angles in radians:
    coneScale = 1 / max(0.001, cos(inner) - cos(outer)), coneOffset = -cos(outer) * coneScale, each operation in float32.  The
    light is full inside the inner cone, dark outside the outer one and f * f of f = clamp(cos * coneScale + coneOffset, 0, 1)
    between them."""
    ci, co = np.float32(np.cos(np.float32(inner_rad))), np.float32(np.cos(np.float32(outer_rad)))
    scale = np.float32(1.0) / np.maximum(np.float32(0.001), np.float32(ci - co))
    return np.float32(scale), np.float32(np.float32(-co) * scale)


def _light_index(who, index):
    return _count(who, index, "index must be a non-negative integer")


def _path_light_count(who, light_count):
    return _count(who, light_count, "light_count must be an integer from 0 to %d (MAX_PATH_LIGHTS)" % MAX_PATH_LIGHTS, MAX_PATH_LIGHTS)


def PunctualLightHits(rays, materials, n, lights, index, lit=None, shadow=True, rays_offset=0, materials_offset=0, lights_offset=0, lit_offset=0,
                      shadow_offset=0):
    """Extension: LightHits for record `index` of the light table `lights`, a device Buffer of PUNCTUAL_LIGHT_DTYPE records that
    begins at lights_offset: directional (as LightHits, bit for bit), point or spot.  The shadow ray towards a point or spot light
    ends at the light (tmax = the distance); a record that is dark at a hit -- out of range, outside the cone, an unknown type --
    gives zeros in `lit` and `shadow`, as does a record whose `hit` is not 1.  lit / shadow as for LightHits.  Returns
    (lit, shadow)."""
    _buffers("PunctualLightHits", rays=rays, materials=materials, lights=lights)
    n, index = int(n), _light_index("PunctualLightHits", index)
    lit, shadow = _lit_and_shadow("PunctualLightHits", n, lit, lit_offset, shadow, shadow_offset)
    _check(_lib.lib().rdx_punctual_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, lights.handle,
                                              int(lights_offset) + _RECORDS["light"][0] * index, lit.handle, int(lit_offset), _h(shadow),
                                              int(shadow_offset)))
    return lit, shadow


def _light_hits_tensors(who, rays_t, materials_t, table, kind, what):
    """the preamble of the two per-hit calls on a light table of tensors: the table -- looked at before the rays, so a refusal of a bad
    table names it --, the rays on its device, the materials -> the _TorchCall and the records of the table"""
    t = _TorchCall(who)
    count = _cuda_tensor(who, table, kind, what)
    t.first(rays_t, "ray", "rays", table.device, what)
    t.also(materials_t, "material", "materials")
    return t, count


def PunctualLightHitsTorch(rays_t, materials_t, lights_t, index, want_shadow=True):
    """Extension: PunctualLightHits on CUDA tensors -- rays and materials as for LightHitsTorch, lights a contiguous float32 (L, 16)
    tensor of PUNCTUAL_LIGHT_DTYPE records (`.view(torch.int32)` shows `type` in column 3), index < L.  Returns (lit, shadow) as
    LightHitsTorch.  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    t, count = _light_hits_tensors("PunctualLightHitsTorch", rays_t, materials_t, lights_t, "light", "lights")
    index = _light_index("PunctualLightHitsTorch", index)
    if index >= count:
        raise RadianceError("PunctualLightHitsTorch: index %d is not one of the %d records of the table" % (index, count))
    lit, shadow = t.new("float4"), t.new("ray", want_shadow)
    if t.begin():
        table = t.wrap(lights_t, "light", count)
        PunctualLightHits(t.wrap(rays_t, "ray"), t.wrap(materials_t, "material"), t.n, table, index, t.wrap(lit, "float4"), t.wrap(shadow, "ray"))
    return lit, shadow


def TracePunctualPaths(tlas, rays, keys, n, max_depth, lights, light_count, scene_buffers, radiance=None, rays_offset=0, keys_offset=0, lights_offset=0,
                       radiance_offset=0):
    """Extension: TraceLightPaths with the first `light_count` (0 .. MAX_PATH_LIGHTS) records of the light table `lights` -- a device
    Buffer of PUNCTUAL_LIGHT_DTYPE records that begins at lights_offset -- sampled at every hit in the place of the scene's
    directional lights: the path tracer over QueryRays / ResolveHits / ResolveMaterials / PunctualLightHits / ScatterHits in one
    call, with its bits.  The table is read on the device by every call; scene_buffers.scene is still required, its lights are not
    read.  Everything else as for TraceLightPaths.  Returns (radiance, invalid)."""
    sb, n = _path_arguments("TracePunctualPaths", n, max_depth, scene_buffers, tlas=tlas, rays=rays, keys=keys, lights=lights)
    light_count = _path_light_count("TracePunctualPaths", light_count)
    radiance = _out_buffer("TracePunctualPaths", n, radiance, radiance_offset, "float4", "radiance", False, flags=False)
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_trace_paths_punctual(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), lights.handle,
                                               int(lights_offset), light_count, C.byref(sb), radiance.handle, int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TracePunctualPathsTorch(tlas, rays_t, keys_t, max_depth, lights_t, scene_buffers):
    """Extension: TracePunctualPaths on CUDA tensors -- rays and keys as for TraceLightPathsTorch, lights a contiguous float32
    (L, 16) tensor of PUNCTUAL_LIGHT_DTYPE records, L <= MAX_PATH_LIGHTS: every record is sampled.  Returns radiance float32
    (n, 4): rgb, 0.  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    # the table is looked at before the rays, so a refusal of a bad table names it
    count = _path_light_count("TracePunctualPathsTorch", _cuda_tensor("TracePunctualPathsTorch", lights_t, "light", "lights"))
    t = _TorchCall("TracePunctualPathsTorch")
    t.first(rays_t, "ray", "rays", lights_t.device, "lights")
    t.also(keys_t, "key", "keys")
    _count("TracePunctualPathsTorch", max_depth, "max_depth must be a non-negative integer")
    radiance = t.new("float4")
    if t.begin():
        # an empty table has no address to wrap: one record of zeros stands in, and none of it is read
        table_t = lights_t if count else t.torch.zeros((1, 16), dtype=t.torch.float32, device=t.device)
        table = t.wrap(table_t, "light", max(count, 1))
        TracePunctualPaths(tlas, t.wrap(rays_t, "ray"), t.wrap(keys_t, "key"), t.n, max_depth, table, count, scene_buffers, t.wrap(radiance, "float4"))
    return radiance


# ---- quad and triangle area lights from a second table of the caller's (rdx_area_light_hits, rdx_trace_paths_area) ---------
AREA_LIGHT_DTYPE = np.dtype([("corner", "<f4", 3), ("type", "<u4"), ("edgeU", "<f4", 3), ("flags", "<u4"), ("edgeV", "<f4", 3), ("_0", "<f4"),
                             ("radiance", "<f4", 3), ("_1", "<f4")])
assert AREA_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_area_light) == 64
_record("area light", AREA_LIGHT_DTYPE, "float32")
AREA_QUAD, AREA_TRIANGLE = 0, 1
AREA_TWO_SIDED = 1       # flags bit 0
MAX_AREA_STREAM = 0xfffe


def _area_record(type, corner, edge_u, edge_v, radiance, two_sided):
    r = np.zeros((), AREA_LIGHT_DTYPE)
    r["type"], r["corner"], r["edgeU"], r["edgeV"], r["radiance"] = type, corner, edge_u, edge_v, radiance
    r["flags"] = AREA_TWO_SIDED if two_sided else 0
    return r


def QuadLight(corner, edge_u, edge_v, radiance, two_sided=False):
    """one AREA_LIGHT_DTYPE record: the parallelogram corner + s * edge_u + t * edge_v, s, t in [0, 1], of constant `radiance`.  It
    emits into the half-space that cross(edge_u, edge_v) points into (a quad under a ceiling with edge_u = +x, edge_v = +z shines
    down) and is dark from behind; two_sided: it emits from both faces."""
    return _area_record(AREA_QUAD, corner, edge_u, edge_v, radiance, two_sided)


def TriangleLight(corner, edge_u, edge_v, radiance, two_sided=False):
    """one AREA_LIGHT_DTYPE record: the triangle corner, corner + edge_u, corner + edge_v; everything else as QuadLight"""
    return _area_record(AREA_TRIANGLE, corner, edge_u, edge_v, radiance, two_sided)


def _area_stream(who, stream, index):
    return _count(who, index if stream is None else stream, "stream must be an integer from 0 to %d" % MAX_AREA_STREAM, MAX_AREA_STREAM)


def AreaLightHits(rays, materials, n, lights, index, keys=None, randoms=None, stream=None, lit=None, shadow=True, rays_offset=0, materials_offset=0,
                  lights_offset=0, keys_offset=0, randoms_offset=0, lit_offset=0, shadow_offset=0):
    """Extension: PunctualLightHits for record `index` of the AREA light table `lights`, a device Buffer of AREA_LIGHT_DTYPE records
    (QuadLight / TriangleLight) that begins at lights_offset.  The emitter is sampled at one point per ray: the random pair is
    pcg3d(frameID, pixel, depth + ((stream + 1) << 16)).xy of the SHADE_KEY_DTYPE records of `keys` -- `stream` defaults to `index`,
    which is what TraceAreaPaths uses -- or, keys None, x and y of the float4 records of `randoms`: exactly one of the two is given.
    The shadow ray stops at 0.999 of the distance to the sampled point; a record that is dark at a hit -- the back face of a
    one-sided emitter, a degenerate emitter, an unknown type -- gives zeros in `lit` and `shadow`, as does a record whose `hit` is
    not 1.  lit / shadow as for LightHits.  Returns (lit, shadow)."""
    _buffers("AreaLightHits", rays=rays, materials=materials, lights=lights)
    hk, hr = _keys_or_randoms("AreaLightHits", keys, randoms)
    n, index = int(n), _light_index("AreaLightHits", index)
    stream = _area_stream("AreaLightHits", stream, index if keys is not None else 0)
    lit, shadow = _lit_and_shadow("AreaLightHits", n, lit, lit_offset, shadow, shadow_offset)
    _check(_lib.lib().rdx_area_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, lights.handle,
                                          int(lights_offset) + _RECORDS["area light"][0] * index, hk, int(keys_offset), stream, hr,
                                          int(randoms_offset), lit.handle, int(lit_offset), _h(shadow), int(shadow_offset)))
    return lit, shadow


def AreaLightHitsTorch(rays_t, materials_t, area_t, index, keys=None, randoms=None, stream=None, want_shadow=True):
    """Extension: AreaLightHits on CUDA tensors -- rays and materials as for LightHitsTorch, area_t a contiguous float32 (A, 16)
    tensor of AREA_LIGHT_DTYPE records (`.view(torch.int32)` shows `type` in column 3 and `flags` in column 7), index < A, and
    exactly one of keys, a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0), and randoms, a contiguous float32 (n, 4)
    tensor (x, y used).  Returns (lit, shadow) as LightHitsTorch.  The library cannot see torch's stream, so the current stream is
    synchronised first; the call blocks."""
    t, count = _light_hits_tensors("AreaLightHitsTorch", rays_t, materials_t, area_t, "area light", "area lights")
    t.keys_or_randoms(keys, randoms)
    index = _light_index("AreaLightHitsTorch", index)
    if index >= count:
        raise RadianceError("AreaLightHitsTorch: index %d is not one of the %d records of the table" % (index, count))
    stream = _area_stream("AreaLightHitsTorch", stream, index if keys is not None else 0)
    lit, shadow = t.new("float4"), t.new("ray", want_shadow)
    if t.begin():
        table = t.wrap(area_t, "area light", count)
        AreaLightHits(t.wrap(rays_t, "ray"), t.wrap(materials_t, "material"), t.n, table, index, t.wrap(keys, "key"), t.wrap(randoms, "float4"), stream,
                      t.wrap(lit, "float4"), t.wrap(shadow, "ray"))
    return lit, shadow


def _area_path_counts(who, light_count, area_count):
    for what, c in (("light_count", light_count), ("area_count", area_count)):
        _count(who, c, "%s must be a non-negative integer" % what)
    if light_count + area_count > MAX_PATH_LIGHTS:
        raise RadianceError("%s: light_count + area_count must not exceed %d (MAX_PATH_LIGHTS)" % (who, MAX_PATH_LIGHTS))
    return int(light_count), int(area_count)


def TraceAreaPaths(tlas, rays, keys, n, max_depth, lights, light_count, area, area_count, scene_buffers, radiance=None, rays_offset=0, keys_offset=0,
                   lights_offset=0, area_offset=0, radiance_offset=0):
    """Extension: TracePunctualPaths over TWO tables: at every hit the first `light_count` PUNCTUAL_LIGHT_DTYPE records of `lights`,
    then the first `area_count` AREA_LIGHT_DTYPE records of `area` -- record j sampled at one point with stream j and the path's
    own (frameID, pixel, depth) --, folded in that order: the path tracer over QueryRays / ResolveHits / ResolveMaterials /
    PunctualLightHits / AreaLightHits / ScatterHits in one call, with its bits.  light_count + area_count <= MAX_PATH_LIGHTS; a
    table whose count is 0 may be None.  With area_count 0 the result has the bits of TracePunctualPaths.  The emitters are not
    geometry: no ray sees them.  Everything else as for TracePunctualPaths.  Returns (radiance, invalid)."""
    sb, n = _path_arguments("TraceAreaPaths", n, max_depth, scene_buffers, tlas=tlas, rays=rays, keys=keys)
    light_count, area_count = _area_path_counts("TraceAreaPaths", light_count, area_count)
    for what, b, c in (("lights", lights, light_count), ("area", area, area_count)):
        if not (isinstance(b, Buffer) or (b is None and c == 0)):
            raise RadianceError("TraceAreaPaths: %s must be a Buffer (or None with a count of 0)" % what)
    radiance = _out_buffer("TraceAreaPaths", n, radiance, radiance_offset, "float4", "radiance", False, flags=False)
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_trace_paths_area(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), _h(lights),
                                           int(lights_offset), light_count, _h(area), int(area_offset), area_count, C.byref(sb), radiance.handle,
                                           int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TraceAreaPathsTorch(tlas, rays_t, keys_t, max_depth, lights_t, area_t, scene_buffers):
    """Extension: TraceAreaPaths on CUDA tensors -- rays and keys as for TraceLightPathsTorch, lights_t a contiguous float32 (L, 16)
    tensor of PUNCTUAL_LIGHT_DTYPE records or None, area_t a contiguous float32 (A, 16) tensor of AREA_LIGHT_DTYPE records or None,
    L + A <= MAX_PATH_LIGHTS: every record is sampled.  Returns radiance float32 (n, 4): rgb, 0.  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks."""
    # the tables are looked at before the rays, so a refusal of a bad table names it
    L = _cuda_tensor("TraceAreaPathsTorch", lights_t, "light", "lights") if lights_t is not None else 0
    A = _cuda_tensor("TraceAreaPathsTorch", area_t, "area light", "area lights") if area_t is not None else 0
    L, A = _area_path_counts("TraceAreaPathsTorch", L, A)
    t = _TorchCall("TraceAreaPathsTorch")
    t.first(rays_t, "ray", "rays")
    for what, table in (("lights", lights_t), ("area lights", area_t)):
        if table is not None and table.device != t.device:
            raise RadianceError("TraceAreaPathsTorch: %s must be on the rays' device" % what)
    t.also(keys_t, "key", "keys")
    _count("TraceAreaPathsTorch", max_depth, "max_depth must be a non-negative integer")
    radiance = t.new("float4")
    if t.begin():
        TraceAreaPaths(tlas, t.wrap(rays_t, "ray"), t.wrap(keys_t, "key"), t.n, max_depth, t.wrap(lights_t, "light", L) if L else None, L,
                       t.wrap(area_t, "area light", A) if A else None, A, scene_buffers, t.wrap(radiance, "float4"))      # an empty table has no address to wrap
    return radiance


# the derived traversal layout (csrc/rdx_types.h), in the order rdx_debug_accel_layout returns its arrays
_DNODE = np.dtype([("bmin", "<f4", 4), ("bmax", "<f4", 4), ("w", "<u4", 4)])
_DWIDE = np.dtype([("lmin", "<f4", 3), ("ld0", "<u4"), ("lmax", "<f4", 3), ("ld1", "<u4"), ("rmin", "<f4", 3), ("rd0", "<u4"),
                   ("rmax", "<f4", 3), ("rd1", "<u4")])
ACCEL_ARRAYS = (("tnodes", _DNODE), ("ctnodes", _DNODE),
                ("insts", np.dtype([("inv", "<f4", 16), ("fwd", "<f4", 16), ("SBTOffset", "<u4"), ("instanceID", "<u4"),
                                    ("customInstanceID", "<u4"), ("blasRoot", "<u4"), ("rootDesc0", "<u4"), ("rootDesc1", "<u4"),
                                    ("_p0", "<u4"), ("_p1", "<u4"), ("rootMin", "<f4", 4), ("rootMax", "<f4", 4),
                                    ("worldMin", "<f4", 4), ("worldMax", "<f4", 4)])),
                ("bnodes", _DNODE),
                ("tris", np.dtype([("v0", "<f4", 3), ("primID", "<u4"), ("e1", "<f4", 3), ("_p0", "<u4"), ("e2", "<f4", 3), ("_p1", "<u4")])),
                ("wide", _DWIDE), ("quad", np.dtype([("half", _DWIDE, 2)])), ("groupBits", np.dtype("<u4")))


def DebugAccelLayout(blob, quad=1, cull=-1, lib=None):
    """Test seam: the traversal layout derived from a TLAS blob under options "quad" / "cull", on the host (no device, no
    Platform) -> (dict of the rdx_accel_scalars members, dict name -> structured array).  `lib`: another build of the library."""
    L = lib if lib is not None else _lib.lib()
    blob = bytes(blob)

    def call(*args):
        if L.rdx_debug_accel_layout(blob, len(blob), int(quad), int(cull), *args) != 0:
            raise RadianceError(L.rdx_last_error().decode("utf-8", "replace"))
    return _layout_from(call)


def DebugAccelLayoutUpdate(blobs, quad=1, cull=-1):
    """Test seam (rdx_debug_accel_layout_update): blobs[0] derived afresh, then updated through blobs[1:] the way UpdateAccelStruct
    updates a device's layout -> (scalars, arrays, [path per step: 1 incremental, 2 full derivation]) of the last blob."""
    L = _lib.lib()
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    ptrs = (C.c_char_p * n)(*blobs)
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    paths = (C.c_uint32 * max(n - 1, 1))()

    def call(*args):
        if L.rdx_debug_accel_layout_update(ptrs, lens, n, int(quad), int(cull), *args, paths) != 0:
            raise RadianceError(L.rdx_last_error().decode("utf-8", "replace"))
    scalars, arrays = _layout_from(call)
    return scalars, arrays, [int(paths[i]) for i in range(n - 1)]


def DebugAccelEntries(blobs, quad=1, cull=-1):
    """Test seam (rdx_debug_accel_entries): the entry records of the layout of blobs[-1] -- one quad record per instance slot, which
    the runtime uploads behind the quad records -- and the pool need of a walk that starts at one -> (structured array, need).
    `blobs`: one blob, or a list that is derived and then updated like DebugAccelLayoutUpdate's."""
    L = _lib.lib()
    blobs = [bytes(blobs)] if isinstance(blobs, (bytes, bytearray, memoryview)) else [bytes(b) for b in blobs]
    n = len(blobs)
    ptrs = (C.c_char_p * n)(*blobs)
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    size, need = C.c_size_t(0), C.c_uint32(0)
    dt = dict(ACCEL_ARRAYS)["quad"]
    if L.rdx_debug_accel_entries(ptrs, lens, n, int(quad), int(cull), None, C.byref(size), C.byref(need)) != 0:
        raise RadianceError(L.rdx_last_error().decode("utf-8", "replace"))
    out = np.zeros(size.value // dt.itemsize, dt)
    if L.rdx_debug_accel_entries(ptrs, lens, n, int(quad), int(cull), out.ctypes.data if out.size else None, C.byref(size), C.byref(need)) != 0:
        raise RadianceError(L.rdx_last_error().decode("utf-8", "replace"))
    return out, int(need.value)


def _layout_from(call):
    """(scalars, arrays) through a seam with the output convention of rdx_debug_accel_layout: a size query, then the arrays"""
    sc = _lib.rdx_accel_scalars()
    sizes = (C.c_size_t * 8)()
    call(C.byref(sc), None, sizes)
    arrays = {}
    for (name, dt), n in zip(ACCEL_ARRAYS, sizes):
        assert n % dt.itemsize == 0, (name, n)
        arrays[name] = np.zeros(n // dt.itemsize, dt)
    ptrs = (C.c_void_p * 8)(*[a.ctypes.data if a.size else None for a in arrays.values()])
    call(None, ptrs, sizes)
    scalars = {n: (list(getattr(sc, n)) if n.startswith("scene") else int(getattr(sc, n))) for n, _ in sc._fields_}
    return scalars, arrays


def MaterialBatch(hits, ray_dirs, pixels, frame_ids, depths):
    h = np.ascontiguousarray(hits, HIT_DTYPE)
    d = np.ascontiguousarray(ray_dirs, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(pixels, np.uint32)
    f = np.ascontiguousarray(frame_ids, np.uint32)
    dp = np.ascontiguousarray(depths, np.int32)
    out = np.zeros(h.shape[0], PAYLOAD_DTYPE)
    _check(_lib.lib().rdx_material_batch(h.ctypes.data, d.ctypes.data, p.ctypes.data, f.ctypes.data, dp.ctypes.data,
                                         h.shape[0], out.ctypes.data))
    return out


def GenerateBatch(pixels, rand_inputs):
    p = np.ascontiguousarray(pixels, np.uint32)
    r = np.ascontiguousarray(rand_inputs, np.uint32).reshape(-1, 3)
    o = np.zeros((p.shape[0], 3), np.float32)
    d = np.zeros((p.shape[0], 3), np.float32)
    _check(_lib.lib().rdx_generate_batch(p.ctypes.data, r.ctypes.data, p.shape[0], o.ctypes.data, d.ctypes.data))
    return o, d


def Pcg3dBatch(inputs):
    r = np.ascontiguousarray(inputs, np.uint32).reshape(-1, 3)
    out = np.zeros((r.shape[0], 3), np.float32)
    _check(_lib.lib().rdx_pcg3d_batch(r.ctypes.data, out.ctypes.data, r.shape[0]))
    return out
