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


# ---- ray queries on device memory (rdx_query_rays) ---------------------------------------------------------------
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("hit", "<u4"), ("primitiveIndex", "<u4"),
                          ("instanceIndex", "<u4"), ("instanceCustomIndex", "<u4"), ("instanceSBTOffset", "<u4")])
assert RAY_DTYPE.itemsize == C.sizeof(_lib.rdx_ray) == 32 and RAY_HIT_DTYPE.itemsize == C.sizeof(_lib.rdx_ray_hit) == 32
QUERY_CLOSEST, QUERY_ANY = 1, 2


def QueryRays(tlas, rays, n, kind=QUERY_CLOSEST, hits=None, rays_offset=0, hits_offset=0):
    """Extension: `n` rays (RAY_DTYPE records, each with its own tmin / tmax) from the device buffer `rays` at byte `rays_offset`
    against `tlas`; one RAY_HIT_DTYPE record per ray goes to the device buffer `hits` at byte `hits_offset` (created when None:
    hits_offset + 32 n bytes).  kind: QUERY_CLOSEST (sbtRecordOffset 1) or QUERY_ANY (2: only `hit` is meaningful).  Nothing
    passes through the host.  Returns `hits`."""
    if not isinstance(rays, Buffer) or not isinstance(tlas, Buffer):
        raise RadianceError("QueryRays: tlas and rays must be Buffers (CreateBuffer / WrapDeviceMemory)")
    if hits is None:
        hits = CreateBuffer(None, max(int(hits_offset) + RAY_HIT_DTYPE.itemsize * int(n), 1))
    elif not isinstance(hits, Buffer):
        raise RadianceError("QueryRays: hits must be a Buffer or None")
    _check(_lib.lib().rdx_query_rays(tlas.handle, rays.handle, int(rays_offset), int(n), int(kind), hits.handle, int(hits_offset)))
    return hits


def _cuda_tensor(who, t, dtypes, shape, what, device=None, owner="rays"):
    """-> n, the rows of `t`: a contiguous CUDA tensor of one of `dtypes` and of `shape` (shape[0] None: any n), on `device` (the
    device of the owner's tensor) if one is given; anything else is a RadianceError"""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.dim() == len(shape) and tuple(t.shape[1:]) == tuple(shape[1:])
            and shape[0] in (None, t.shape[0]) and t.is_contiguous() and (device is None or t.device == device)):
        raise RadianceError("%s: %s must be a contiguous %s CUDA tensor of shape (n,%s)%s"
                            % (who, what, " / ".join(str(d).replace("torch.", "") for d in dtypes), "".join(" %d" % s for s in shape[1:]),
                               " on the %s' device" % owner if device is not None else ""))
    return int(t.shape[0])


def QueryRaysTorch(tlas, rays_tensor, kind=QUERY_CLOSEST, out=None):
    """Extension: rays from a contiguous float32 CUDA tensor of shape (n, 8) -- origin, tmin, direction, tmax per row; the records
    land in `out`, an int32 (or float32) CUDA tensor of shape (n, 8) (created when None: int32; `.view(torch.float32)` shows t,
    b1, b2).  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    import torch
    t = rays_tensor
    n = _cuda_tensor("QueryRaysTorch", t, (torch.float32,), (None, 8), "rays")
    if out is None:
        out = torch.empty((n, 8), dtype=torch.int32, device=t.device)
    else:
        _cuda_tensor("QueryRaysTorch", out, (torch.int32, torch.float32), (n, 8), "out", t.device)
    torch.cuda.current_stream(t.device).synchronize()
    if n:
        rays = WrapDeviceMemory(None, t.data_ptr(), n * 32, keepalive=t)
        hits = WrapDeviceMemory(None, out.data_ptr(), n * 32, keepalive=out)
        QueryRays(tlas, rays, n, kind, hits)
    return out


# ---- surface records of a query's hits (rdx_resolve_hits) ----------------------------------------------------------
SURFACE_DTYPE = np.dtype([("position", "<f4", 3), ("hit", "<u4"), ("normal", "<f4", 3), ("materialIndex", "<u4"),
                          ("above", "<f4", 3), ("u", "<f4"), ("below", "<f4", 3), ("v", "<f4")])
assert SURFACE_DTYPE.itemsize == C.sizeof(_lib.rdx_surface) == 64


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
    if not (isinstance(tlas, Buffer) and isinstance(rays, Buffer) and isinstance(hits, Buffer)):
        raise RadianceError("ResolveHits: tlas, rays and hits must be Buffers (CreateBuffer / WrapDeviceMemory)")
    if not isinstance(scene_buffers, SurfaceBuffers):
        try:
            scene_buffers = SurfaceBuffers(*scene_buffers)
        except TypeError:
            raise RadianceError("ResolveHits: scene_buffers must be a SurfaceBuffers or a (meshInfo, index, uv, normal) tuple")
    sb = scene_buffers._struct()
    if out is None:
        out = CreateBuffer(None, max(int(out_offset) + SURFACE_DTYPE.itemsize * int(n), 1))
    elif not isinstance(out, Buffer):
        raise RadianceError("ResolveHits: out must be a Buffer or None")
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_resolve_hits(tlas.handle, rays.handle, int(rays_offset), hits.handle, int(hits_offset), int(n), C.byref(sb),
                                       out.handle, int(out_offset), C.byref(invalid)))
    return out, int(invalid.value)


def ResolveHitsTorch(tlas, rays_tensor, hits_tensor, scene_buffers, out=None):
    """Extension: ResolveHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32 (n, 8)
    tensor QueryRaysTorch returned for them; the records land in `out`, a contiguous float32 CUDA tensor of shape (n, 16)
    (created when None; `.view(torch.int32)` shows hit and materialIndex in columns 3 and 7).  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks.  Returns (out, invalid)."""
    import torch
    r, h = rays_tensor, hits_tensor
    n = _cuda_tensor("ResolveHitsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("ResolveHitsTorch", h, (torch.int32, torch.float32), (n, 8), "hits", r.device)
    if out is None:
        out = torch.empty((n, 16), dtype=torch.float32, device=r.device)
    else:
        _cuda_tensor("ResolveHitsTorch", out, (torch.float32,), (n, 16), "out", r.device)
    torch.cuda.current_stream(r.device).synchronize()
    invalid = 0
    if n:
        rays = WrapDeviceMemory(None, r.data_ptr(), n * 32, keepalive=r)
        hits = WrapDeviceMemory(None, h.data_ptr(), n * 32, keepalive=h)
        dst = WrapDeviceMemory(None, out.data_ptr(), n * 64, keepalive=out)
        _, invalid = ResolveHits(tlas, rays, hits, n, scene_buffers, dst)
    return out, invalid


def DebugSurfaceInBounds(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, nmeshinfo=None):
    """Test seam (rdx_debug_surface_in_bounds): the bounds rule of ResolveHits for one record, on the host -> bool.  meshInfo: a
    MeshInfo array (nmeshinfo defaults to its length), idx3: the triangle's three vertex numbers or None."""
    mi = np.ascontiguousarray(meshInfo, MeshInfo).reshape(-1)
    nm = mi.shape[0] if nmeshinfo is None else int(nmeshinfo)
    iv = None if idx3 is None else (C.c_uint32 * 3)(*[int(x) & 0xffffffff for x in idx3])
    rc = _lib.lib().rdx_debug_surface_in_bounds(mi.ctypes.data_as(C.POINTER(_lib.rdx_mesh_info)), int(ninst), nm, int(instanceIndex) & 0xffffffff,
                                                int(primitiveIndex) & 0xffffffff, iv, int(nindex), int(nnormal), int(nuv))
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
        h = lambda x: x.handle if x is not None else None
        return _lib.rdx_shading_buffers(self.scene.handle, self.meshInfo.handle, self.index.handle, h(self.uv), self.normal.handle,
                                        self.material.handle, h(self.textureArray), h(self.sampler))


def _shading_struct(who, scene_buffers):
    """the rdx_shading_buffers of a ShadingBuffers, or of a tuple of its constructor's arguments"""
    if not isinstance(scene_buffers, ShadingBuffers):
        try:
            scene_buffers = ShadingBuffers(*scene_buffers)
        except TypeError:
            raise RadianceError("%s: scene_buffers must be a ShadingBuffers or a (scene, meshInfo, index, uv, normal, material"
                                "[, textureArray, sampler]) tuple" % who)
    return scene_buffers._struct(who)


def _out_buffer(who, n, buf, offset, rec, what, optional, or_true=None):
    """an output argument: a Buffer; True, or None where it is not optional: created for n records of `rec` bytes behind `offset`;
    None / False where it is optional: not wanted.  or_true: the refusal names True as a choice (default: where optional)"""
    if buf is True or (buf is None and not optional):
        return CreateBuffer(None, max(int(offset) + rec * n, 1))
    if buf is None or buf is False:
        return None
    if not isinstance(buf, Buffer):
        raise RadianceError("%s: %s must be a Buffer%s" % (who, what, ", True or None" if (optional if or_true is None else or_true) else " or None"))
    return buf


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
    if not all(isinstance(b, Buffer) for b in (tlas, rays, hits, keys)):
        raise RadianceError("ShadeHits: tlas, rays, hits and keys must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("ShadeHits", scene_buffers)
    n = int(n)
    shade = _out_buffer("ShadeHits", n, shade, shade_offset, SHADE_DTYPE.itemsize, "shade", False)
    next = _out_buffer("ShadeHits", n, next, next_offset, RAY_DTYPE.itemsize, "next", True)
    shadow = _out_buffer("ShadeHits", n, shadow, shadow_offset, RAY_DTYPE.itemsize, "shadow", True)
    src = _out_buffer("ShadeHits", n, True if (src is None and compact) else src, src_offset, 4, "src", True)
    live, invalid = C.c_uint32(0), C.c_uint32(0)
    h = lambda b: b.handle if b is not None else None
    _check(_lib.lib().rdx_shade_hits(tlas.handle, rays.handle, int(rays_offset), hits.handle, int(hits_offset), keys.handle, int(keys_offset), n,
                                     C.byref(sb), shade.handle, int(shade_offset), h(next), int(next_offset), h(shadow), int(shadow_offset),
                                     h(src), int(src_offset), C.byref(live), C.byref(invalid)))
    return shade, next, shadow, src, int(live.value), int(invalid.value)


def ShadeHitsTorch(tlas, rays_t, hits_t, keys_t, scene_buffers, compact=True, sample_next=True):
    """Extension: ShadeHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32 (n, 8)
    tensor QueryRaysTorch returned for them, keys a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0).  Returns (shade,
    next, shadow, src, live, invalid): shade float32 (n, 12) (`.view(torch.int32)` shows hit, materialIndex and slot in columns 3,
    7, 11), next / shadow float32 (live, 8) when compacting -- already sliced to the survivors -- else (n, 8), src int32 (live,)
    or None; next is None without sample_next.  The library cannot see torch's stream, so the current stream is synchronised
    first; the call blocks."""
    import torch
    r, h, k = rays_t, hits_t, keys_t
    n = _cuda_tensor("ShadeHitsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("ShadeHitsTorch", h, (torch.int32, torch.float32), (n, 8), "hits", r.device)
    _cuda_tensor("ShadeHitsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    shade = torch.empty((n, 12), dtype=torch.float32, device=r.device)
    nxt = torch.empty((n, 8), dtype=torch.float32, device=r.device) if sample_next else None
    shadow = torch.empty((n, 8), dtype=torch.float32, device=r.device)
    src = torch.empty((n,), dtype=torch.int32, device=r.device) if compact else None
    torch.cuda.current_stream(r.device).synchronize()
    live = invalid = 0
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        _, _, _, _, live, invalid = ShadeHits(tlas, wrap(r, 32), wrap(h, 32), wrap(k, 16), n, scene_buffers, wrap(shade, 48), wrap(nxt, 32),
                                              wrap(shadow, 32), wrap(src, 4))
    if compact:
        nxt, shadow, src = (nxt[:live] if nxt is not None else None), shadow[:live], src[:live]
    return shade, nxt, shadow, src, live, invalid


def DebugShadeInBounds(meshInfo, ninst, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv, materials, textures=False, layers=0,
                       nmeshinfo=None, nmaterials=None):
    """Test seam (rdx_debug_shade_in_bounds): the bounds rule of ShadeHits for one record, on the host -> bool.  As
    DebugSurfaceInBounds, plus `materials`: a Material array (nmaterials defaults to its length), textures: texels are read,
    layers: layers of the image array."""
    mi = np.ascontiguousarray(meshInfo, MeshInfo).reshape(-1)
    mt = np.ascontiguousarray(materials, Material).reshape(-1)
    nm = mi.shape[0] if nmeshinfo is None else int(nmeshinfo)
    nmat = mt.shape[0] if nmaterials is None else int(nmaterials)
    iv = None if idx3 is None else (C.c_uint32 * 3)(*[int(x) & 0xffffffff for x in idx3])
    rc = _lib.lib().rdx_debug_shade_in_bounds(mi.ctypes.data_as(C.POINTER(_lib.rdx_mesh_info)), int(ninst), nm, int(instanceIndex) & 0xffffffff,
                                              int(primitiveIndex) & 0xffffffff, iv, int(nindex), int(nnormal), int(nuv),
                                              mt.ctypes.data_as(C.POINTER(_lib.rdx_material)), nmat, 1 if textures else 0, int(layers))
    if rc < 0:
        raise RadianceError(_lib.last_error())
    return rc == 1


# ---- the evaluated material of a query's hits, and one light's direct term (rdx_resolve_materials, rdx_light_hits) --------
MATERIAL_RECORD_DTYPE = np.dtype([("normal", "<f4", 3), ("hit", "<u4"), ("albedo", "<f4", 3), ("materialIndex", "<u4"), ("metallic", "<f4"),
                                  ("roughness", "<f4"), ("transmission", "<f4"), ("ior", "<f4"), ("above", "<f4", 3), ("_0", "<u4")])
assert MATERIAL_RECORD_DTYPE.itemsize == C.sizeof(_lib.rdx_material_record) == 64
MAX_LIGHTS = 5          # the DirLights of a SceneProperties


def ResolveMaterials(tlas, rays, hits, n, scene_buffers, out=None, rays_offset=0, hits_offset=0, out_offset=0):
    """Extension: one MATERIAL_RECORD_DTYPE record per ray -- the shading normal (normal map applied), the sampled albedo, metallic,
    roughness, transmission, ior, the shadow ray's origin `above` and the material number, as the stock closest-hit shader holds
    them -- for the `n` RAY_HIT_DTYPE records QueryRays(..., QUERY_CLOSEST) wrote to `hits` for `rays`; device buffers in, device
    buffer out (created when None: out_offset + 64 n bytes).  scene_buffers: a ShadingBuffers or a tuple of its constructor's
    arguments, textures by ShadeHits' rule.  Misses are 64 zero bytes; so are hits that would read outside a scene buffer, which
    are counted.  Returns (out, invalid)."""
    if not (isinstance(tlas, Buffer) and isinstance(rays, Buffer) and isinstance(hits, Buffer)):
        raise RadianceError("ResolveMaterials: tlas, rays and hits must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("ResolveMaterials", scene_buffers)
    if out is None:
        out = CreateBuffer(None, max(int(out_offset) + MATERIAL_RECORD_DTYPE.itemsize * int(n), 1))
    elif not isinstance(out, Buffer):
        raise RadianceError("ResolveMaterials: out must be a Buffer or None")
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
    if not all(isinstance(b, Buffer) for b in (rays, materials, scene)):
        raise RadianceError("LightHits: rays, materials and scene must be Buffers (CreateBuffer / WrapDeviceMemory)")
    n, light = int(n), int(light)
    if not 0 <= light < MAX_LIGHTS:
        raise RadianceError("LightHits: light %d is not one of the %d lights of a SceneProperties (0 .. %d)" % (light, MAX_LIGHTS, MAX_LIGHTS - 1))
    if lit is None:
        lit = CreateBuffer(None, max(int(lit_offset) + 16 * n, 1))
    elif not isinstance(lit, Buffer):
        raise RadianceError("LightHits: lit must be a Buffer or None")
    shadow = _out_buffer("LightHits", n, shadow, shadow_offset, RAY_DTYPE.itemsize, "shadow", True)
    _check(_lib.lib().rdx_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, scene.handle, light, lit.handle,
                                     int(lit_offset), shadow.handle if shadow is not None else None, int(shadow_offset)))
    return lit, shadow


def ResolveMaterialsTorch(tlas, rays_tensor, hits_tensor, scene_buffers, out=None):
    """Extension: ResolveMaterials on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, hits the contiguous int32 / float32
    (n, 8) tensor QueryRaysTorch returned for them; the records land in `out`, a contiguous float32 CUDA tensor of shape (n, 16)
    (created when None): columns 0-2 the normal, 4-6 the albedo, 8-11 metallic, roughness, transmission, ior, 12-14 `above`;
    `.view(torch.int32)` shows hit and materialIndex in columns 3 and 7.  The library cannot see torch's stream, so the current
    stream is synchronised first; the call blocks.  Returns (out, invalid)."""
    import torch
    r, h = rays_tensor, hits_tensor
    n = _cuda_tensor("ResolveMaterialsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("ResolveMaterialsTorch", h, (torch.int32, torch.float32), (n, 8), "hits", r.device)
    if out is None:
        out = torch.empty((n, 16), dtype=torch.float32, device=r.device)
    else:
        _cuda_tensor("ResolveMaterialsTorch", out, (torch.float32,), (n, 16), "out", r.device)
    torch.cuda.current_stream(r.device).synchronize()
    invalid = 0
    if n:
        rays = WrapDeviceMemory(None, r.data_ptr(), n * 32, keepalive=r)
        hits = WrapDeviceMemory(None, h.data_ptr(), n * 32, keepalive=h)
        dst = WrapDeviceMemory(None, out.data_ptr(), n * 64, keepalive=out)
        _, invalid = ResolveMaterials(tlas, rays, hits, n, scene_buffers, dst)
    return out, invalid


def LightHitsTorch(rays_t, materials_t, scene_buffer, light, want_shadow=True):
    """Extension: LightHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, materials the contiguous float32 (n, 16)
    tensor ResolveMaterialsTorch returned for them (or the caller's own records), scene_buffer the Buffer of descriptor slot 4.
    Returns (lit, shadow): lit float32 (n, 4) (rgb, 0), shadow float32 (n, 8) -- the rays QueryRaysTorch(..., QUERY_ANY) takes --
    or None without want_shadow.  The library cannot see torch's stream, so the current stream is synchronised first; the call
    blocks."""
    import torch
    r, m = rays_t, materials_t
    n = _cuda_tensor("LightHitsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("LightHitsTorch", m, (torch.float32,), (n, 16), "materials", r.device)
    if not isinstance(scene_buffer, Buffer):
        raise RadianceError("LightHitsTorch: scene_buffer must be a Buffer (the SceneProperties of descriptor slot 4)")
    light = int(light)
    if not 0 <= light < MAX_LIGHTS:
        raise RadianceError("LightHitsTorch: light %d is not one of the %d lights of a SceneProperties (0 .. %d)" % (light, MAX_LIGHTS, MAX_LIGHTS - 1))
    lit = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    shadow = torch.empty((n, 8), dtype=torch.float32, device=r.device) if want_shadow else None
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        LightHits(wrap(r, 32), wrap(m, 64), n, scene_buffer, light, wrap(lit, 16), wrap(shadow, 32))
    return lit, shadow


# ---- the next ray of a query's hits from material and surface records (rdx_scatter_hits) --------------------------------
SCATTER_DTYPE = np.dtype([("nextFactor", "<f4", 3), ("slot", "<u4")])
assert SCATTER_DTYPE.itemsize == C.sizeof(_lib.rdx_scatter) == 16


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
    if not all(isinstance(b, Buffer) for b in (rays, materials, surfaces)):
        raise RadianceError("ScatterHits: rays, materials and surfaces must be Buffers (CreateBuffer / WrapDeviceMemory)")
    for what, b in (("keys", keys), ("randoms", randoms)):
        if b is not None and not isinstance(b, Buffer):
            raise RadianceError("ScatterHits: %s must be a Buffer or None" % what)
    if keys is None and randoms is None:
        raise RadianceError("ScatterHits: neither keys nor randoms given: one of the two is required")
    if keys is not None and randoms is not None:
        raise RadianceError("ScatterHits: both keys and randoms given: only one of the two is allowed")
    n = int(n)
    scatter = _out_buffer("ScatterHits", n, scatter, scatter_offset, SCATTER_DTYPE.itemsize, "scatter", False)
    next = _out_buffer("ScatterHits", n, next, next_offset, RAY_DTYPE.itemsize, "next", False)
    src = _out_buffer("ScatterHits", n, True if (src is None and compact) else src, src_offset, 4, "src", True, or_true=False)
    live = C.c_uint32(0)
    h = lambda b: b.handle if b is not None else None
    _check(_lib.lib().rdx_scatter_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), surfaces.handle, int(surfaces_offset),
                                       h(keys), int(keys_offset), h(randoms), int(randoms_offset), n, scatter.handle, int(scatter_offset),
                                       next.handle, int(next_offset), h(src), int(src_offset), C.byref(live)))
    return scatter, next, src, int(live.value)


def ScatterHitsTorch(rays_t, materials_t, surfaces_t, keys_t=None, randoms_t=None, compact=True):
    """Extension: ScatterHits on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, materials / surfaces the contiguous float32
    (n, 16) tensors ResolveMaterialsTorch / ResolveHitsTorch returned for them (or the caller's own records), and exactly one of
    keys, a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0), and randoms, a contiguous float32 (n, 4) tensor (xyz used).
    Returns (scatter, next, src, live): scatter float32 (n, 4) (nextFactor; `.view(torch.int32)` shows slot in column 3), next
    float32 (live, 8) when compacting -- already sliced to the survivors -- else (n, 8), src int32 (live,) or None.  The library
    cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, m, s, k, u = rays_t, materials_t, surfaces_t, keys_t, randoms_t
    n = _cuda_tensor("ScatterHitsTorch", r, (torch.float32,), (None, 8), "rays")
    for what, t in (("materials", m), ("surfaces", s)):
        _cuda_tensor("ScatterHitsTorch", t, (torch.float32,), (n, 16), what, r.device)
    if (k is None) == (u is None):
        raise RadianceError("ScatterHitsTorch: exactly one of keys and randoms must be given")
    if k is not None:
        _cuda_tensor("ScatterHitsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    if u is not None:
        _cuda_tensor("ScatterHitsTorch", u, (torch.float32,), (n, 4), "randoms", r.device)
    scatter = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    nxt = torch.empty((n, 8), dtype=torch.float32, device=r.device)
    src = torch.empty((n,), dtype=torch.int32, device=r.device) if compact else None
    torch.cuda.current_stream(r.device).synchronize()
    live = 0
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        _, _, _, live = ScatterHits(wrap(r, 32), wrap(m, 64), wrap(s, 64), wrap(k, 16), n, wrap(u, 16), wrap(scatter, 16), wrap(nxt, 32), wrap(src, 4))
    if compact:
        nxt, src = nxt[:live], src[:live]
    return scatter, nxt, src, live


# ---- the two ends of a frame on device memory (rdx_generate_rays, rdx_accumulate) ---------------------------------------
RAYGEN_SEED_DTYPE = np.dtype([("in", "<u4", 3), ("_0", "<u4")])
assert RAYGEN_SEED_DTYPE.itemsize == C.sizeof(_lib.rdx_raygen_seed) == 16
ACCUMULATE_DEBUG = 1


def _optional_buffer(who, buf, what):
    if buf is not None and not isinstance(buf, Buffer):
        raise RadianceError("%s: %s must be a Buffer or None" % (who, what))
    return buf.handle if buf is not None else None


def GenerateRays(camera, n, frame_id, total_samples, first_pixel=0, pixels=None, seeds=None, tmin=0.001, tmax=1000.0, rays=None, keys=True,
                 pixels_offset=0, seeds_offset=0, rays_offset=0, keys_offset=0):
    """Extension: `n` camera rays of the PhysicalCamera in the device buffer `camera` (the contents of descriptor slot 3; it need
    not be bound, and is read on the device by every call), as RAY_DTYPE records in `rays` -- ready for QueryRays -- and
    SHADE_KEY_DTYPE records (frame_id, pixel, 0, 0) in `keys` -- the keys of depth 0 for ShadeHits.  Ray i belongs to pixel
    first_pixel + i, or pixels[i] (`pixels`: a Buffer of uint32); its random input is pcg3d(frame_id, total_samples, pixel) as in
    the reference's raygen, or pcg3d of seeds[i] (`seeds`: a Buffer of RAYGEN_SEED_DTYPE).  Every ray has the bits of the frame
    path's generateRay; tmin / tmax are written as given.  rays: a Buffer, or None (created).  keys: a Buffer, True (created) or
    None / False (not wanted).  Nothing passes through the host.  Returns (rays, keys)."""
    if not isinstance(camera, Buffer):
        raise RadianceError("GenerateRays: camera must be a Buffer (CreateBuffer / WrapDeviceMemory)")
    n = int(n)
    if rays is None:
        rays = CreateBuffer(None, max(int(rays_offset) + RAY_DTYPE.itemsize * n, 1))
    elif not isinstance(rays, Buffer):
        raise RadianceError("GenerateRays: rays must be a Buffer or None")
    if keys is True:
        keys = CreateBuffer(None, max(int(keys_offset) + SHADE_KEY_DTYPE.itemsize * n, 1))
    elif keys is False:
        keys = None
    hp, hs, hk = (_optional_buffer("GenerateRays", b, w) for b, w in ((pixels, "pixels"), (seeds, "seeds"), (keys, "keys")))
    _check(_lib.lib().rdx_generate_rays(camera.handle, n, int(first_pixel), hp, int(pixels_offset), int(frame_id), int(total_samples), hs,
                                        int(seeds_offset), float(tmin), float(tmax), rays.handle, int(rays_offset), hk, int(keys_offset)))
    return rays, keys


def GenerateRaysTorch(camera, n_or_pixels, frame_id, total_samples, seeds=None):
    """Extension: GenerateRays into CUDA tensors.  n_or_pixels: an int n (pixels 0 .. n - 1), or a contiguous int32 CUDA tensor of
    pixel numbers, shape (n,).  seeds: None, or a contiguous int32 CUDA tensor of shape (n, 4) (the three inputs of pcg3d, 0).
    Returns (rays float32 (n, 8): origin, tmin = 0.001, direction, tmax = 1000 per row -- what QueryRaysTorch takes; keys int32
    (n, 4): frame_id, pixel, 0, 0 -- what ShadeHitsTorch takes at depth 0).  The library cannot see torch's stream, so the
    current stream is synchronised first; the call blocks."""
    import torch
    px = None
    if isinstance(n_or_pixels, torch.Tensor):
        px = n_or_pixels
        n, device = _cuda_tensor("GenerateRaysTorch", px, (torch.int32,), (None,), "pixels"), px.device
    elif isinstance(n_or_pixels, (int, np.integer)) and not isinstance(n_or_pixels, bool) and n_or_pixels >= 0:
        n, device = int(n_or_pixels), torch.device("cuda", torch.cuda.current_device())
    else:
        raise RadianceError("GenerateRaysTorch: the second argument is a ray count or an int32 CUDA tensor of pixel numbers")
    if seeds is not None:
        _cuda_tensor("GenerateRaysTorch", seeds, (torch.int32,), (n, 4), "seeds", device, owner="pixels")
    rays = torch.empty((n, 8), dtype=torch.float32, device=device)
    keys = torch.empty((n, 4), dtype=torch.int32, device=device)
    torch.cuda.current_stream(device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        GenerateRays(camera, n, frame_id, total_samples, 0, wrap(px, 4), wrap(seeds, 16), rays=wrap(rays, 32), keys=wrap(keys, 16))
    return rays, keys


def Accumulate(colors, n, frame_id, scratch, image=None, first_pixel=0, pixels=None, debug=False, colors_offset=0, pixels_offset=0):
    """Extension: the end of a frame's sample on the device.  colors: a Buffer of `n` float4 records (rgb, w ignored), sample
    `frame_id` of pixels first_pixel + i, or pixels[i] (`pixels`: a Buffer of uint32).  scratch (imageScratch, float4 per pixel)
    takes the reference's running mean -- rgb = colour for frame_id 0, else (frame_id * rgb + colour) / (frame_id + 1) in
    float32, w kept -- and image (RGBA8, optional) the tone-mapped mean of those pixels (debug: no ACES, no gamma).  One call is
    one frame_id; its pixels must be distinct (of two samples of one pixel one wins, unspecified which).  Returns `invalid`:
    the samples whose pixel number is not below min(scratch.size / 16, image.size / 4); they write nothing."""
    if not isinstance(colors, Buffer) or not isinstance(scratch, Buffer):
        raise RadianceError("Accumulate: colors and scratch must be Buffers (CreateBuffer / WrapDeviceMemory)")
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
    import torch
    c = colors
    n = _cuda_tensor("AccumulateTorch", c, (torch.float32,), (None, 4), "colors")
    if pixels is not None:
        _cuda_tensor("AccumulateTorch", pixels, (torch.int32,), (n,), "pixels", c.device, owner="colours")

    def frame(t, dtype, what):
        if t is None or isinstance(t, Buffer):
            return t
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == 4 and t.is_contiguous()
                and t.device == c.device):
            raise RadianceError("AccumulateTorch: %s must be a Buffer or a contiguous %s CUDA tensor of shape (npix, 4) on the colours' device"
                                % (what, str(dtype).replace("torch.", "")))
        return WrapDeviceMemory(None, t.data_ptr(), t.numel() * t.element_size(), keepalive=t) if t.numel() else None
    if scratch is None:
        raise RadianceError("AccumulateTorch: scratch must be a Buffer or a float32 CUDA tensor of shape (npix, 4)")
    bs, bi = frame(scratch, torch.float32, "scratch"), frame(image, torch.uint8, "image")
    torch.cuda.current_stream(c.device).synchronize()
    if not n:
        return 0
    if bs is None or (image is not None and bi is None):       # a frame of no pixels: every sample is outside it
        return n
    wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
    return Accumulate(wrap(c, 16), n, frame_id, bs, bi, 0, wrap(pixels, 4), debug)


# ---- radiance along the caller's own rays (rdx_trace_paths) -------------------------------------------------------------
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
    if not all(isinstance(b, Buffer) for b in (tlas, rays, keys)):
        raise RadianceError("TracePaths: tlas, rays and keys must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("TracePaths", scene_buffers)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) \
            or max_depth < 0:
        raise RadianceError("TracePaths: n and max_depth must be non-negative integers")
    n = int(n)
    if radiance is None:
        radiance = CreateBuffer(None, max(int(radiance_offset) + 16 * n, 1))
    elif not isinstance(radiance, Buffer):
        raise RadianceError("TracePaths: radiance must be a Buffer or None")
    made_hits = hits is True
    if made_hits:
        hits = CreateBuffer(None, max(int(hits_offset) + RAY_HIT_DTYPE.itemsize * n, 1))
    elif hits is False:
        hits = None
    hh = _optional_buffer("TracePaths", hits, "hits")
    _check(_lib.lib().rdx_trace_paths(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), C.byref(sb),
                                      radiance.handle, int(radiance_offset), hh, int(hits_offset)))
    return (radiance, hits) if made_hits else radiance


def TracePathsTorch(tlas, rays_t, keys_t, max_depth, scene_buffers, want_hits=False):
    """Extension: TracePaths on CUDA tensors -- rays a contiguous float32 (n, 8) tensor (origin, tmin, direction, tmax per row), keys
    a contiguous int32 (n, 4) tensor (frameID, pixel, -, -): what GenerateRaysTorch returns, or rays of the caller's own.
    Returns radiance float32 (n, 4): rgb, 0 -- what AccumulateTorch takes -- and, with want_hits, (radiance, hits int32 (n, 8)).
    The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, k = rays_t, keys_t
    n = _cuda_tensor("TracePathsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("TracePathsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or max_depth < 0:
        raise RadianceError("TracePathsTorch: max_depth must be a non-negative integer")
    radiance = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    hits = torch.empty((n, 8), dtype=torch.int32, device=r.device) if want_hits else None
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        TracePaths(tlas, wrap(r, 32), wrap(k, 16), n, max_depth, scene_buffers, wrap(radiance, 16), wrap(hits, 32))
    return (radiance, hits) if want_hits else radiance


# ---- radiance along the caller's own rays, every light of the scene sampled (rdx_trace_paths_lights) ---------------------
def _light_count(who, light_count):
    if isinstance(light_count, bool) or not isinstance(light_count, (int, np.integer)) or not 0 <= light_count <= 5:
        raise RadianceError("%s: light_count must be an integer from 0 to 5 (the lights of a SceneProperties)" % who)
    return int(light_count)


def TraceLightPaths(tlas, rays, keys, n, max_depth, light_count, scene_buffers, radiance=None, rays_offset=0, keys_offset=0, radiance_offset=0):
    """Extension: TracePaths with the first `light_count` (0 .. 5) directional lights of scene_buffers.scene sampled at every hit --
    the path tracer over QueryRays / ResolveHits / ResolveMaterials / LightHits / ScatterHits (the README's second loop) in one
    call, with its bits.  Rays and keys as for TracePaths.  The lights are read on the device by every call.  The call gathers
    checked: a hit that scene_buffers does not describe is a miss and is counted.  radiance: a Buffer, or None (created:
    radiance_offset + 16 n bytes).  Device buffers in and out.  Returns (radiance, invalid)."""
    if not all(isinstance(b, Buffer) for b in (tlas, rays, keys)):
        raise RadianceError("TraceLightPaths: tlas, rays and keys must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("TraceLightPaths", scene_buffers)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) \
            or max_depth < 0:
        raise RadianceError("TraceLightPaths: n and max_depth must be non-negative integers")
    light_count = _light_count("TraceLightPaths", light_count)
    n = int(n)
    if radiance is None:
        radiance = CreateBuffer(None, max(int(radiance_offset) + 16 * n, 1))
    elif not isinstance(radiance, Buffer):
        raise RadianceError("TraceLightPaths: radiance must be a Buffer or None")
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_trace_paths_lights(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), light_count,
                                             C.byref(sb), radiance.handle, int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TraceLightPathsTorch(tlas, rays_t, keys_t, max_depth, light_count, scene_buffers):
    """Extension: TraceLightPaths on CUDA tensors -- rays a contiguous float32 (n, 8) tensor, keys a contiguous int32 (n, 4) tensor, as
    for TracePathsTorch.  Returns radiance float32 (n, 4): rgb, 0 -- what AccumulateTorch takes.  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, k = rays_t, keys_t
    n = _cuda_tensor("TraceLightPathsTorch", r, (torch.float32,), (None, 8), "rays")
    _cuda_tensor("TraceLightPathsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or max_depth < 0:
        raise RadianceError("TraceLightPathsTorch: max_depth must be a non-negative integer")
    light_count = _light_count("TraceLightPathsTorch", light_count)
    radiance = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t)
        TraceLightPaths(tlas, wrap(r, 32), wrap(k, 16), n, max_depth, light_count, scene_buffers, wrap(radiance, 16))
    return radiance


# ---- point and spot lights from a caller's light table (rdx_punctual_light_hits, rdx_trace_paths_punctual) -----------------
PUNCTUAL_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("type", "<u4"), ("direction", "<f4", 3), ("range", "<f4"), ("color", "<f4", 3),
                                 ("_0", "<f4"), ("coneScale", "<f4"), ("coneOffset", "<f4"), ("_1", "<f4"), ("_2", "<f4")])
assert PUNCTUAL_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_punctual_light) == 64
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


def _light_index(who, index, what="index"):
    if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or index < 0:
        raise RadianceError("%s: %s must be a non-negative integer" % (who, what))
    return int(index)


def _path_light_count(who, light_count):
    if isinstance(light_count, bool) or not isinstance(light_count, (int, np.integer)) or not 0 <= light_count <= MAX_PATH_LIGHTS:
        raise RadianceError("%s: light_count must be an integer from 0 to %d (MAX_PATH_LIGHTS)" % (who, MAX_PATH_LIGHTS))
    return int(light_count)


def PunctualLightHits(rays, materials, n, lights, index, lit=None, shadow=True, rays_offset=0, materials_offset=0, lights_offset=0, lit_offset=0,
                      shadow_offset=0):
    """Extension: LightHits for record `index` of the light table `lights`, a device Buffer of PUNCTUAL_LIGHT_DTYPE records that
    begins at lights_offset: directional (as LightHits, bit for bit), point or spot.  The shadow ray towards a point or spot light
    ends at the light (tmax = the distance); a record that is dark at a hit -- out of range, outside the cone, an unknown type --
    gives zeros in `lit` and `shadow`, as does a record whose `hit` is not 1.  lit / shadow as for LightHits.  Returns
    (lit, shadow)."""
    if not all(isinstance(b, Buffer) for b in (rays, materials, lights)):
        raise RadianceError("PunctualLightHits: rays, materials and lights must be Buffers (CreateBuffer / WrapDeviceMemory)")
    n, index = int(n), _light_index("PunctualLightHits", index)
    if lit is None:
        lit = CreateBuffer(None, max(int(lit_offset) + 16 * n, 1))
    elif not isinstance(lit, Buffer):
        raise RadianceError("PunctualLightHits: lit must be a Buffer or None")
    shadow = _out_buffer("PunctualLightHits", n, shadow, shadow_offset, RAY_DTYPE.itemsize, "shadow", True)
    _check(_lib.lib().rdx_punctual_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, lights.handle,
                                              int(lights_offset) + PUNCTUAL_LIGHT_DTYPE.itemsize * index, lit.handle, int(lit_offset),
                                              shadow.handle if shadow is not None else None, int(shadow_offset)))
    return lit, shadow


def _light_table_tensor(who, lights_t):
    """an (L, 16) float32 CUDA tensor of PUNCTUAL_LIGHT_DTYPE records -> L.  The table is looked at before the rays, so a refusal
    of a bad table names it"""
    import torch
    return _cuda_tensor(who, lights_t, (torch.float32,), (None, 16), "lights")


def PunctualLightHitsTorch(rays_t, materials_t, lights_t, index, want_shadow=True):
    """Extension: PunctualLightHits on CUDA tensors -- rays and materials as for LightHitsTorch, lights a contiguous float32 (L, 16)
    tensor of PUNCTUAL_LIGHT_DTYPE records (`.view(torch.int32)` shows `type` in column 3), index < L.  Returns (lit, shadow) as
    LightHitsTorch.  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, m = rays_t, materials_t
    count = _light_table_tensor("PunctualLightHitsTorch", lights_t)
    n = _cuda_tensor("PunctualLightHitsTorch", r, (torch.float32,), (None, 8), "rays", lights_t.device, "lights")
    _cuda_tensor("PunctualLightHitsTorch", m, (torch.float32,), (n, 16), "materials", r.device)
    index = _light_index("PunctualLightHitsTorch", index)
    if index >= count:
        raise RadianceError("PunctualLightHitsTorch: index %d is not one of the %d records of the table" % (index, count))
    lit = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    shadow = torch.empty((n, 8), dtype=torch.float32, device=r.device) if want_shadow else None
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        table = WrapDeviceMemory(None, lights_t.data_ptr(), count * 64, keepalive=lights_t)
        PunctualLightHits(wrap(r, 32), wrap(m, 64), n, table, index, wrap(lit, 16), wrap(shadow, 32))
    return lit, shadow


def TracePunctualPaths(tlas, rays, keys, n, max_depth, lights, light_count, scene_buffers, radiance=None, rays_offset=0, keys_offset=0, lights_offset=0,
                       radiance_offset=0):
    """Extension: TraceLightPaths with the first `light_count` (0 .. MAX_PATH_LIGHTS) records of the light table `lights` -- a device
    Buffer of PUNCTUAL_LIGHT_DTYPE records that begins at lights_offset -- sampled at every hit in the place of the scene's
    directional lights: the path tracer over QueryRays / ResolveHits / ResolveMaterials / PunctualLightHits / ScatterHits in one
    call, with its bits.  The table is read on the device by every call; scene_buffers.scene is still required, its lights are not
    read.  Everything else as for TraceLightPaths.  Returns (radiance, invalid)."""
    if not all(isinstance(b, Buffer) for b in (tlas, rays, keys, lights)):
        raise RadianceError("TracePunctualPaths: tlas, rays, keys and lights must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("TracePunctualPaths", scene_buffers)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) \
            or max_depth < 0:
        raise RadianceError("TracePunctualPaths: n and max_depth must be non-negative integers")
    light_count = _path_light_count("TracePunctualPaths", light_count)
    n = int(n)
    if radiance is None:
        radiance = CreateBuffer(None, max(int(radiance_offset) + 16 * n, 1))
    elif not isinstance(radiance, Buffer):
        raise RadianceError("TracePunctualPaths: radiance must be a Buffer or None")
    invalid = C.c_uint32(0)
    _check(_lib.lib().rdx_trace_paths_punctual(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), lights.handle,
                                               int(lights_offset), light_count, C.byref(sb), radiance.handle, int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TracePunctualPathsTorch(tlas, rays_t, keys_t, max_depth, lights_t, scene_buffers):
    """Extension: TracePunctualPaths on CUDA tensors -- rays and keys as for TraceLightPathsTorch, lights a contiguous float32
    (L, 16) tensor of PUNCTUAL_LIGHT_DTYPE records, L <= MAX_PATH_LIGHTS: every record is sampled.  Returns radiance float32
    (n, 4): rgb, 0.  The library cannot see torch's stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, k = rays_t, keys_t
    count = _path_light_count("TracePunctualPathsTorch", _light_table_tensor("TracePunctualPathsTorch", lights_t))
    n = _cuda_tensor("TracePunctualPathsTorch", r, (torch.float32,), (None, 8), "rays", lights_t.device, "lights")
    _cuda_tensor("TracePunctualPathsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or max_depth < 0:
        raise RadianceError("TracePunctualPathsTorch: max_depth must be a non-negative integer")
    radiance = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t)
        # an empty table has no address to wrap: one record of zeros stands in, and none of it is read
        table_t = lights_t if count else torch.zeros((1, 16), dtype=torch.float32, device=r.device)
        table = WrapDeviceMemory(None, table_t.data_ptr(), max(count, 1) * 64, keepalive=table_t)
        TracePunctualPaths(tlas, wrap(r, 32), wrap(k, 16), n, max_depth, table, count, scene_buffers, wrap(radiance, 16))
    return radiance


# ---- quad and triangle area lights from a second table of the caller's (rdx_area_light_hits, rdx_trace_paths_area) ---------
AREA_LIGHT_DTYPE = np.dtype([("corner", "<f4", 3), ("type", "<u4"), ("edgeU", "<f4", 3), ("flags", "<u4"), ("edgeV", "<f4", 3), ("_0", "<f4"),
                             ("radiance", "<f4", 3), ("_1", "<f4")])
assert AREA_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_area_light) == 64
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
    if stream is None:
        stream = index
    if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= stream <= MAX_AREA_STREAM:
        raise RadianceError("%s: stream must be an integer from 0 to %d" % (who, MAX_AREA_STREAM))
    return int(stream)


def AreaLightHits(rays, materials, n, lights, index, keys=None, randoms=None, stream=None, lit=None, shadow=True, rays_offset=0, materials_offset=0,
                  lights_offset=0, keys_offset=0, randoms_offset=0, lit_offset=0, shadow_offset=0):
    """Extension: PunctualLightHits for record `index` of the AREA light table `lights`, a device Buffer of AREA_LIGHT_DTYPE records
    (QuadLight / TriangleLight) that begins at lights_offset.  The emitter is sampled at one point per ray: the random pair is
    pcg3d(frameID, pixel, depth + ((stream + 1) << 16)).xy of the SHADE_KEY_DTYPE records of `keys` -- `stream` defaults to `index`,
    which is what TraceAreaPaths uses -- or, keys None, x and y of the float4 records of `randoms`: exactly one of the two is given.
    The shadow ray stops at 0.999 of the distance to the sampled point; a record that is dark at a hit -- the back face of a
    one-sided emitter, a degenerate emitter, an unknown type -- gives zeros in `lit` and `shadow`, as does a record whose `hit` is
    not 1.  lit / shadow as for LightHits.  Returns (lit, shadow)."""
    if not all(isinstance(b, Buffer) for b in (rays, materials, lights)):
        raise RadianceError("AreaLightHits: rays, materials and lights must be Buffers (CreateBuffer / WrapDeviceMemory)")
    for what, b in (("keys", keys), ("randoms", randoms)):
        if b is not None and not isinstance(b, Buffer):
            raise RadianceError("AreaLightHits: %s must be a Buffer or None" % what)
    if keys is None and randoms is None:
        raise RadianceError("AreaLightHits: neither keys nor randoms given: one of the two is required")
    if keys is not None and randoms is not None:
        raise RadianceError("AreaLightHits: both keys and randoms given: only one of the two is allowed")
    n, index = int(n), _light_index("AreaLightHits", index)
    stream = _area_stream("AreaLightHits", stream, index if keys is not None else 0)
    if lit is None:
        lit = CreateBuffer(None, max(int(lit_offset) + 16 * n, 1))
    elif not isinstance(lit, Buffer):
        raise RadianceError("AreaLightHits: lit must be a Buffer or None")
    shadow = _out_buffer("AreaLightHits", n, shadow, shadow_offset, RAY_DTYPE.itemsize, "shadow", True)
    h = lambda b: b.handle if b is not None else None
    _check(_lib.lib().rdx_area_light_hits(rays.handle, int(rays_offset), materials.handle, int(materials_offset), n, lights.handle,
                                          int(lights_offset) + AREA_LIGHT_DTYPE.itemsize * index, h(keys), int(keys_offset), stream, h(randoms),
                                          int(randoms_offset), lit.handle, int(lit_offset), h(shadow), int(shadow_offset)))
    return lit, shadow


def AreaLightHitsTorch(rays_t, materials_t, area_t, index, keys=None, randoms=None, stream=None, want_shadow=True):
    """Extension: AreaLightHits on CUDA tensors -- rays and materials as for LightHitsTorch, area_t a contiguous float32 (A, 16)
    tensor of AREA_LIGHT_DTYPE records (`.view(torch.int32)` shows `type` in column 3 and `flags` in column 7), index < A, and
    exactly one of keys, a contiguous int32 (n, 4) tensor (frameID, pixel, depth, 0), and randoms, a contiguous float32 (n, 4)
    tensor (x, y used).  Returns (lit, shadow) as LightHitsTorch.  The library cannot see torch's stream, so the current stream is
    synchronised first; the call blocks."""
    import torch
    r, m = rays_t, materials_t
    count = _cuda_tensor("AreaLightHitsTorch", area_t, (torch.float32,), (None, 16), "area lights")
    n = _cuda_tensor("AreaLightHitsTorch", r, (torch.float32,), (None, 8), "rays", area_t.device, "area lights")
    _cuda_tensor("AreaLightHitsTorch", m, (torch.float32,), (n, 16), "materials", r.device)
    if (keys is None) == (randoms is None):
        raise RadianceError("AreaLightHitsTorch: exactly one of keys and randoms must be given")
    if keys is not None:
        _cuda_tensor("AreaLightHitsTorch", keys, (torch.int32,), (n, 4), "keys", r.device)
    if randoms is not None:
        _cuda_tensor("AreaLightHitsTorch", randoms, (torch.float32,), (n, 4), "randoms", r.device)
    index = _light_index("AreaLightHitsTorch", index)
    if index >= count:
        raise RadianceError("AreaLightHitsTorch: index %d is not one of the %d records of the table" % (index, count))
    stream = _area_stream("AreaLightHitsTorch", stream, index if keys is not None else 0)
    lit = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    shadow = torch.empty((n, 8), dtype=torch.float32, device=r.device) if want_shadow else None
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t) if t is not None else None
        table = WrapDeviceMemory(None, area_t.data_ptr(), count * 64, keepalive=area_t)
        AreaLightHits(wrap(r, 32), wrap(m, 64), n, table, index, wrap(keys, 16), wrap(randoms, 16), stream, wrap(lit, 16), wrap(shadow, 32))
    return lit, shadow


def _area_path_counts(who, light_count, area_count):
    for what, c in (("light_count", light_count), ("area_count", area_count)):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0:
            raise RadianceError("%s: %s must be a non-negative integer" % (who, what))
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
    if not all(isinstance(b, Buffer) for b in (tlas, rays, keys)):
        raise RadianceError("TraceAreaPaths: tlas, rays and keys must be Buffers (CreateBuffer / WrapDeviceMemory)")
    sb = _shading_struct("TraceAreaPaths", scene_buffers)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0 or isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) \
            or max_depth < 0:
        raise RadianceError("TraceAreaPaths: n and max_depth must be non-negative integers")
    light_count, area_count = _area_path_counts("TraceAreaPaths", light_count, area_count)
    for what, b, c in (("lights", lights, light_count), ("area", area, area_count)):
        if not (isinstance(b, Buffer) or (b is None and c == 0)):
            raise RadianceError("TraceAreaPaths: %s must be a Buffer (or None with a count of 0)" % what)
    n = int(n)
    if radiance is None:
        radiance = CreateBuffer(None, max(int(radiance_offset) + 16 * n, 1))
    elif not isinstance(radiance, Buffer):
        raise RadianceError("TraceAreaPaths: radiance must be a Buffer or None")
    invalid = C.c_uint32(0)
    h = lambda b: b.handle if b is not None else None
    _check(_lib.lib().rdx_trace_paths_area(tlas.handle, rays.handle, int(rays_offset), keys.handle, int(keys_offset), n, int(max_depth), h(lights),
                                           int(lights_offset), light_count, h(area), int(area_offset), area_count, C.byref(sb), radiance.handle,
                                           int(radiance_offset), C.byref(invalid)))
    return radiance, int(invalid.value)


def TraceAreaPathsTorch(tlas, rays_t, keys_t, max_depth, lights_t, area_t, scene_buffers):
    """Extension: TraceAreaPaths on CUDA tensors -- rays and keys as for TraceLightPathsTorch, lights_t a contiguous float32 (L, 16)
    tensor of PUNCTUAL_LIGHT_DTYPE records or None, area_t a contiguous float32 (A, 16) tensor of AREA_LIGHT_DTYPE records or None,
    L + A <= MAX_PATH_LIGHTS: every record is sampled.  Returns radiance float32 (n, 4): rgb, 0.  The library cannot see torch's
    stream, so the current stream is synchronised first; the call blocks."""
    import torch
    r, k = rays_t, keys_t
    L = _light_table_tensor("TraceAreaPathsTorch", lights_t) if lights_t is not None else 0
    A = _cuda_tensor("TraceAreaPathsTorch", area_t, (torch.float32,), (None, 16), "area lights") if area_t is not None else 0
    L, A = _area_path_counts("TraceAreaPathsTorch", L, A)
    n = _cuda_tensor("TraceAreaPathsTorch", r, (torch.float32,), (None, 8), "rays")
    for what, t in (("lights", lights_t), ("area lights", area_t)):
        if t is not None and t.device != r.device:
            raise RadianceError("TraceAreaPathsTorch: %s must be on the rays' device" % what)
    _cuda_tensor("TraceAreaPathsTorch", k, (torch.int32,), (n, 4), "keys", r.device)
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or max_depth < 0:
        raise RadianceError("TraceAreaPathsTorch: max_depth must be a non-negative integer")
    radiance = torch.empty((n, 4), dtype=torch.float32, device=r.device)
    torch.cuda.current_stream(r.device).synchronize()
    if n:
        wrap = lambda t, rec: WrapDeviceMemory(None, t.data_ptr(), n * rec, keepalive=t)
        table = lambda t, c: WrapDeviceMemory(None, t.data_ptr(), c * 64, keepalive=t) if c else None      # an empty table has no address to wrap
        TraceAreaPaths(tlas, wrap(r, 32), wrap(k, 16), n, max_depth, table(lights_t, L), L, table(area_t, A), A, scene_buffers, wrap(radiance, 16))
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
