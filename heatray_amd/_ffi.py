"""The calls of the C-ABI under include/, over the declarations of heatray_amd._abi.

`Engine` drives any shared library that exports the C-ABI of include/hrcore.h under
a given symbol prefix.  The product binds it to libhrcore.so (prefix ``hr_``, see
heatray_amd.core); the test-suite binds the same class to the CPU oracle (prefix
``ora_``) so both are fed identical POD inputs.  Nothing in this package loads the
oracle.
"""
import ctypes as C

import numpy as np

from ._abi import *  # noqa: F401,F403  (every constant, struct and table of the headers is also this module's)


def display_params(tonemapping_enabled=False, exposure=0.0, brightness=0.0, contrast=1.0, hue=1.0, saturation=1.0,
                   vibrance=0.0, red=1.0, green=1.0, blue=1.0, vignette_intensity=0.0, vignette_falloff=1.0):
    """Defaults = the reference's PostProcessingParams defaults; camera_exposure = 2^exposure (computed in binary32 by
    repeated doubling / halving for integral exposures, else through numpy's float32 power, as std::powf would)."""
    return DisplayParams(int(bool(tonemapping_enabled)), float(np.float32(2.0) ** np.float32(exposure)), brightness, contrast, hue,
                         saturation, vibrance, red, green, blue, vignette_intensity, vignette_falloff)


class EngineError(RuntimeError):
    pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, typ=f32p):
    return a.ctypes.data_as(typ) if a is not None else typ()


def _strided(a, comps):
    """(the array as the C-ABI can read it, its stride in bytes): a float32 V x comps array whose last axis is contiguous goes as it
    is, stride included; anything else is packed tight.  None -> (None, 0)."""
    if a is None:
        return None, 0
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != comps or a.strides[1] != 4 or a.strides[0] < 4 * comps:
        a = _f32(a).reshape(-1, comps)
    return a, a.strides[0]


def _image(p, w, h, copy=True):
    """The H x W x 4 float32 image a read-back call left at p (with its size in w, h): a copy, or a view of the library's buffer."""
    a = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4))
    return a.copy() if copy else a


_BOUND = {}


def _bind(lib, prefix):
    """{name: the library's function with the result and argument types of PROTOTYPES}, made once per (lib, prefix).  lib[...] makes
    function objects of our own: the attributes of `lib`, which others may call, stay without prototypes.  A symbol the library lacks
    is left out."""
    if (lib, prefix) not in _BOUND:
        fns = {}
        for prototypes in PROTOTYPES.values():
            for name, argtypes in prototypes.items():
                try:
                    fn = lib[prefix + name]
                except AttributeError:
                    continue
                fn.restype, fn.argtypes = restype(name), argtypes
                fns[name] = fn
        _BOUND[lib, prefix] = fns
    return _BOUND[lib, prefix]


class Engine:
    """Thin object wrapper over one hr_ctx (or ora_ctx)."""

    def __init__(self, lib, prefix, device_id=0, rank=0, world=1, tile_size=32, stream=None, flags=0, memory_budget=0):
        self._init(lib, prefix)
        if "abi_version" not in self._fns:
            raise EngineError(f"{prefix}abi_version missing: the library predates this binding (ABI {HR_ABI_VERSION})")
        self._check_version("abi_version", HR_ABI_VERSION)
        desc = CtxDesc(device_id, rank, world, tile_size, stream, flags, int(memory_budget))
        rc = self._fn("ctx_create")(desc, C.byref(self._ctx))
        if rc != HR_OK:
            self._ctx = C.c_void_p()
            raise EngineError(f"{prefix}ctx_create failed with status {rc} (no usable HIP device, a bad descriptor, or a malformed HR_TUNE: see stderr)")

    # -- plumbing
    def _init(self, lib, prefix):
        """What every engine starts from, before it has a context."""
        self._lib = lib
        self._p = prefix
        self._ctx = C.c_void_p()
        self.width = self.height = 0
        self._fns = _bind(lib, prefix)
        self._features_checked = set()
        self._mesh_vertices = {}  # id -> vertex count (mesh_attribute sizes its output by it)
        self._deform_rigs = {}    # id -> (morphs, joints) of the bound rig (deform_pose checks its inputs against them)

    def _check_version(self, fn, want):
        ver = self._fns[fn]
        if ver() != want:
            raise EngineError(f"{self._p}{fn}() = {ver()}, this binding was written against {want}: rebuild the library")

    def _fn(self, name):
        try:
            return self._fns[name]
        except KeyError:
            raise AttributeError(f"the library has no {self._p}{name}") from None

    def _call(self, name, *args):
        rc = self._fn(name)(self._ctx, *args)
        if rc != HR_OK:
            msg = self._fn("last_error")(self._ctx)
            raise EngineError(f"{self._p}{name}: status {rc}: {msg.decode() if msg else ''}")

    def _feature_call(self, feature, name, *args):
        """_call for an entry point of an optional header (FEATURES).  A feature is checked on its first call: a library without its
        symbols (the CPU oracle) still makes an Engine, and the feature's calls raise EngineError."""
        if feature not in self._features_checked:
            symbols, want, words = FEATURES[feature]
            missing = [s for s in symbols if s not in self._fns]
            if missing:
                raise EngineError(f"this library has no {words} (lacks {[self._p + s for s in missing]})")
            self._check_version(f"{feature}_api_version", want)
            self._features_checked.add(feature)
        self._call(name, *args)

    def close(self):
        if self._ctx:
            self._fn("ctx_destroy")(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- frame
    def resize(self, w, h):
        self._call("frame_resize", w, h)
        self.width, self.height = w, h

    def bind_external_frame(self, device_ptr):
        self._call("frame_bind_external", device_ptr)

    def frame_device_ptr(self):
        p = C.c_void_p()
        self._call("frame_device_ptr", C.byref(p))
        return p.value

    def set_stream(self, stream):
        self._call("ctx_set_stream", stream)

    # -- geometry
    def add_mesh(self, positions, normals, indices, uvs=None, tangents=None, bitangents=None, colors=None,
                 mode=HR_TRIANGLES, world=None, front_face_cw=None, is_occluder=True, material_id=0):
        pos, nrm = _f32(positions).reshape(-1, 3), _f32(normals).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        opt = [None if a is None else _f32(a) for a in (uvs, tangents, bitangents, colors)]
        m = np.eye(4, dtype=np.float32) if world is None else _f32(world).reshape(4, 4)
        if front_face_cw is None:  # Mesh.cpp:86-91: determinant of the full 4x4
            front_face_cw = bool(np.linalg.det(m.astype(np.float64)) < 0)
        d = MeshDesc()
        d.positions, d.normals = _ptr(pos), _ptr(nrm)
        d.uvs, d.tangents, d.bitangents, d.colors = (_ptr(a) for a in opt)
        d.n_vertices = pos.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        # numpy holds the matrix as m[row][col]; the ABI wants column-major storage
        d.world_from_entity = (C.c_float * 16)(*m.T.reshape(-1))
        d.front_face_cw, d.is_occluder, d.material_id = int(front_face_cw), int(is_occluder), material_id
        gid = C.c_int32()
        self._call("geom_add", d, C.byref(gid))
        self._mesh_vertices[gid.value] = d.n_vertices
        return gid.value

    def add_mesh_strided(self, buf, pos_off, nrm_off, uv_off, stride_floats, indices, mode=HR_TRIANGLES, world=None, is_occluder=True,
                         material_id=0):
        """One interleaved float buffer (n, stride_floats) holding positions / normals / uvs at the given float offsets."""
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        d = MeshDesc()
        base = buf.ctypes.data
        d.positions = C.cast(base + 4 * pos_off, f32p)
        d.normals = C.cast(base + 4 * nrm_off, f32p)
        if uv_off is not None:
            d.uvs = C.cast(base + 4 * uv_off, f32p)
        d.position_stride = d.normal_stride = d.uv_stride = 4 * stride_floats
        d.n_vertices = buf.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        m = np.eye(4, dtype=np.float32) if world is None else _f32(world).reshape(4, 4)
        d.world_from_entity = (C.c_float * 16)(*m.T.reshape(-1))
        d.front_face_cw, d.is_occluder, d.material_id = int(np.linalg.det(m.astype(np.float64)) < 0), int(is_occluder), material_id
        gid = C.c_int32(-1)
        self._call("geom_add", d, C.byref(gid))
        self._mesh_vertices[gid.value] = d.n_vertices
        return gid.value

    def remove_mesh(self, gid):
        self._call("geom_remove", gid)
        self._mesh_vertices.pop(gid, None)
        self._deform_rigs.pop(gid, None)

    def set_transform(self, gid, world):
        m = _f32(world).reshape(4, 4)
        self._call("geom_set_transform", gid, (C.c_float * 16)(*m.T.reshape(-1)))

    def clear_scene(self):
        self._call("scene_clear")
        self._mesh_vertices.clear()
        self._deform_rigs.clear()

    def set_scene_cache(self, path):
        self._call("scene_cache", None if not path else str(path).encode())

    def commit(self):
        self._call("scene_commit")

    def scene_info(self):
        s = SceneInfo()
        self._call("scene_get_info", s)
        return s

    def tree_info(self):
        """hr_tree_info of the last commit that built the tree (include/hrcore_tree.h)"""
        t = TreeInfo()
        self._feature_call("tree", "scene_get_tree_info", t)
        return t

    def tree_readback(self):
        """The committed tree as the traversal kernels read it (include/hrcore_tree.h): {"layout": the hr_tree_layout as a dict with
        numpy arrays for its vectors, "node4": (n, 16) uint32, "node32": (n, 8) uint32, "leaf_keys": (n,) int32, "tris": (slots, 12)
        float32 in leaf order, "node_box": (n, 6) float32, "slot_of_prim": (triangles,) uint32}.  tests/tree_audit.py reads it."""
        lay = TreeLayout()
        self._feature_call("tree", "scene_tree_layout", lay)
        out = {"layout": {k: np.array(v) if hasattr(v, "__len__") else v for k, v in lay.as_dict().items()}}
        shapes = (("node4", HR_TREE_NODE4, np.uint32, 16), ("node32", HR_TREE_NODE32, np.uint32, 8), ("leaf_keys", HR_TREE_LEAF_KEYS, np.int32, 0),
                  ("tris", HR_TREE_TRIS, np.float32, 12), ("node_box", HR_TREE_NODE_BOX, np.float32, 6), ("slot_of_prim", HR_TREE_SLOT_OF_PRIM, np.uint32, 0))
        for name, what, dtype, width in shapes:
            a = np.empty(lay.bytes[what] // 4, dtype)
            if a.size:  # (a root leaf has no nodes, an empty scene nothing: the library refuses a null buffer)
                self._feature_call("tree", "scene_tree_read", what, a.ctypes.data, a.nbytes)
            out[name] = a.reshape(-1, width) if width else a
        return out

    # -- textures / materials / lights
    def create_texture(self, pixels, wrap=HR_WRAP_REPEAT, filter=HR_FILTER_LINEAR):
        a = np.ascontiguousarray(pixels)
        if a.ndim == 2:
            a = a[:, :, None]
        dtype = HR_TEX_U8 if a.dtype == np.uint8 else HR_TEX_F32
        if dtype == HR_TEX_F32:
            a = _f32(a)
        d = TextureDesc(a.shape[1], a.shape[0], a.shape[2], dtype, wrap, wrap, filter)
        tid = C.c_int32()
        self._call("texture_create", d, a.ctypes.data, C.byref(tid))
        return tid.value

    def destroy_texture(self, tid):
        self._call("texture_destroy", tid)

    def set_material(self, material_id, material):
        self._call("material_set", material_id, material)

    def set_lights(self, lights):
        self._call("lights_set", lights)

    # -- sample tables
    def set_sequences(self, seq_xy, aperture_xy):
        s, a = _f32(seq_xy), _f32(aperture_xy)
        assert s.shape == a.shape and s.ndim == 3 and s.shape[2] == 2
        self._call("sequences_set", _ptr(s), _ptr(a), s.shape[0], s.shape[1])

    def set_seq_offsets(self, offsets_xy):
        o = _f32(offsets_xy).reshape(-1, 2)
        self._call("seq_offsets_set", _ptr(o), o.shape[0])

    def qmc_generate(self, mode, sequence_index, count, radial=False):
        out = np.empty((count, 2), dtype=np.float32)
        self._call("qmc_generate", mode, sequence_index, count, int(radial), _ptr(out))
        return out

    def aperture_generate(self, bokeh, sequence_index, count):
        """One aperture table as PassGenerator.cpp:653-676 makes it: radialSobol or randomPolygonal(5 / 6 / 8 edges, seed = sequence)."""
        out = np.empty((count, 2), dtype=np.float32)
        self._call("aperture_generate", bokeh, sequence_index, count, _ptr(out))
        return out

    def generate_sequences(self, sample_mode=HR_SAMPLE_SOBOL, bokeh=HR_BOKEH_CIRCULAR, length=32):
        self._call("sequences_generate", sample_mode, bokeh, length)

    def generate_seq_offsets(self):
        self._call("seq_offsets_generate")

    def generate_multiscatter_lut(self, want_host=True):
        out = np.empty((128, 128), dtype=np.float32) if want_host else None
        tid = C.c_int32()
        self._call("multiscatter_lut_generate", _ptr(out), C.byref(tid))
        return out, tid.value

    # -- rendering
    def clear(self):
        self._call("clear")

    def render_pass(self, params):
        self._call("render_pass", params)

    def set_interactive_blocks(self, coords_xy):
        """coords_xy: (ny, nx, 2) integer array in texture memory order, or None for the unshuffled list."""
        if coords_xy is None:
            self._call("interactive_blocks_set", None, 0, 0)
            return
        a = np.ascontiguousarray(coords_xy, dtype=np.int32)
        self._call("interactive_blocks_set", _ptr(a, i32p), a.shape[1], a.shape[0])

    def pass_batch(self, max_ray_depth):
        b = C.c_int32(0)
        self._call("frame_pass_batch", max_ray_depth, C.byref(b))
        return int(b.value)

    def flush(self):
        self._call("flush")

    def stats(self):
        s = PassStats()
        self._call("get_stats", s)
        return s

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since the last clear: HIP-event times (zero unless the context was created with
        HR_CTX_TIME_KERNELS), under "trace_clock" k_trace's time by the device clock (always), under "camera_packets" whether camera
        rays are traced as packets at the moment and the union factor the selector's last probe measured."""
        t = KernelTimes()
        self._call("get_kernel_times", t)
        d = {n: (t.ms[i], t.launches[i]) for i, n in enumerate(HR_KERNEL_NAMES)}
        d["trace_clock"] = (t.trace_clock_ms, t.trace_clock_launches)
        d["camera_packets"] = (bool(t.camera_packets), t.packet_union, t.camera_packets)  # (camera rays as packets now?, the probe's union factor, passes per packet)
        return d

    def step_log(self, capacity=4096):
        """[(start_ms, trace_ms, passes_in_flight, passes_injected, group)] of the macro steps since the last clear (newest 4096), sorted by start."""
        recs = (StepRecord * capacity)()
        n = C.c_int32()
        self._call("get_step_log", recs, capacity, C.byref(n))
        return [(r.start_ms, r.trace_ms, r.passes_in_flight, r.passes_injected, r.group) for r in recs[: n.value]]

    def synchronize(self):
        self._call("synchronize")

    def readback(self, copy=True):
        p = f32p()
        w, h = C.c_int32(), C.c_int32()
        self._call("readback", C.byref(p), C.byref(w), C.byref(h))
        return _image(p, w, h, copy)

    def display(self, params=None, fmt=HR_DISPLAY_RGBA8, with_passes=False):
        """Display resolve of the accumulation buffer -> numpy: uint8 [H, W, 4] (RGBA8) or float32 [H, W, 4];
        with_passes: (image, number of complete passes it shows)."""
        params = params if params is not None else display_params()
        dt, ch = (np.uint8, 4) if (fmt & 0xFF) == HR_DISPLAY_RGBA8 else (np.float32, 4)
        p = C.c_void_p()
        w, h = C.c_int32(), C.c_int32()
        shown = C.c_uint32()
        self._call("display_readback", params, fmt, C.byref(p), C.byref(w), C.byref(h), C.byref(shown))
        n = w.value * h.value * ch
        buf = (C.c_uint8 * n).from_address(p.value) if dt is np.uint8 else (C.c_float * n).from_address(p.value)
        img = np.frombuffer(buf, dtype=dt).reshape(h.value, w.value, ch).copy()
        return (img, int(shown.value)) if with_passes else img

    def passes_resolved(self):
        """Passes added to the accumulation buffer since the last clear, as enqueued so far (no synchronisation)."""
        n = C.c_uint64()
        self._call("frame_passes_resolved", C.byref(n))
        return int(n.value)

    # -- tile-shard exchange (device pointers for the HIP core, host pointers for the oracle)
    def packed_slots(self, rank, world):
        n = C.c_uint64()
        self._call("frame_packed_slots", rank, world, C.byref(n))
        return int(n.value)

    def pack_owned(self, out_ptr, stream=None):
        self._call("frame_pack_owned", int(out_ptr), stream or 0)

    def unpack(self, src_rank, world, packed_ptr, full_ptr, stream=None):
        self._call("frame_unpack", src_rank, world, int(packed_ptr), int(full_ptr), stream or 0)

    def display_device(self, device_ptr, params=None, fmt=HR_DISPLAY_RGBA8):
        """Asynchronous display resolve into device memory (e.g. a torch tensor or a GL-interop buffer)."""
        params = params if params is not None else display_params()
        self._call("display", params, fmt, int(device_ptr), None)

    def readback_progressive(self, copy=True):
        """(buffer, complete passes in it) without completing the passes still in the pipeline.  copy=False returns a view
        of the context's pinned buffer (valid until the next readback)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        self._call("readback_progressive", C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        return _image(p, w, h, copy), int(n.value)

    # -- AOVs (include/hrcore_aov.h)
    def set_aovs(self, mask):
        """Enable the AOV planes of `mask` (HR_AOV_SURFACE | HR_AOV_MOMENTS; 0 frees them).  Completes the passes in flight; a changed
        mask starts the planes at zero, so they hold the passes requested after this call."""
        self._feature_call("aov", "aov_enable", int(mask))

    def aov_mask(self):
        m = C.c_uint32()
        self._feature_call("aov", "aov_mask", C.byref(m))
        return int(m.value)

    def aov_plane(self, plane):
        """(H x W x 4 float32 copy of one plane, passes summed into it); completes the enqueued passes first."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint64()
        self._feature_call("aov", "aov_readback", plane, C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        return _image(p, w, h), int(n.value)

    def aovs(self):
        """The raw sums of every enabled plane: {"albedo", "normal_depth", "moments": H x W x 4 float32, "passes": n}
        (include/hrcore_aov.h; heatray_amd.aov.resolve turns them into means and a variance)."""
        mask = self.aov_mask()
        out = {}
        for plane, name in enumerate(AOV_PLANE_NAMES):
            if mask & (HR_AOV_MOMENTS if plane == HR_AOV_PLANE_MOMENTS else HR_AOV_SURFACE):
                out[name], out["passes"] = self.aov_plane(plane)
        return out

    def aov_to_device(self, plane, device_ptr, stream=None):
        """Asynchronous copy of one plane (W x H float4) into device memory, e.g. a torch tensor; ordered like display_device."""
        self._feature_call("aov", "aov_copy", plane, int(device_ptr), stream or 0)

    # -- denoiser (include/hrcore_denoise.h)
    def denoise(self, params=None, with_passes=False):
        """The denoised frame (H x W x 4 float32: rgb = mean colour, a = 1) of the passes rendered so far; needs both AOV masks enabled
        before the frame's first pass.  params: a DenoiseParams (heatray_amd.denoise.default_params()), None = the defaults."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        self._feature_call("denoise", "denoise_readback", params, C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        img = _image(p, w, h)
        return (img, int(n.value)) if with_passes else img

    def denoise_to_device(self, device_ptr, params=None, stream=None):
        """Asynchronous: the denoised frame (W x H float4) into device memory, e.g. a torch tensor; ordered like aov_to_device."""
        self._feature_call("denoise", "denoise", params, int(device_ptr), stream or 0, None)

    def denoise_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None):
        """Asynchronous display resolve of the denoised frame into device memory (like display_device)."""
        display = display if display is not None else display_params()
        self._feature_call("denoise", "denoise_display", params, display, fmt, int(device_ptr), None)

    # -- denoiser with the spatial variance estimate (include/hrcore_denoise_spatial.h)
    def denoise_spatial(self, params=None, spatial=None, with_result=False):
        """denoise() with a spatial variance estimate for the pixels that have fewer than spatial.below samples (one-sample pixels no
        longer pass through unfiltered).  params: a DenoiseParams, spatial: a DenoiseSpatialParams
        (heatray_amd.denoise_spatial.default_params()); None = the defaults.  with_result: (image, the DenoiseSpatialResult as a dict)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DenoiseSpatialResult()
        self._feature_call("denoise_spatial", "denoise_spatial_readback", params, spatial, C.byref(p), C.byref(w), C.byref(h), C.byref(n), r)
        img = _image(p, w, h)
        return (img, r.as_dict()) if with_result else img

    def denoise_spatial_to_device(self, device_ptr, params=None, spatial=None, stream=None):
        """Asynchronous: denoise_spatial's image (W x H float4) into device memory; ordered like denoise_to_device."""
        self._feature_call("denoise_spatial", "denoise_spatial", params, spatial, int(device_ptr), stream or 0, None, None)

    def denoise_spatial_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None, spatial=None):
        """Asynchronous display resolve of denoise_spatial's image into device memory (like denoise_display)."""
        display = display if display is not None else display_params()
        self._feature_call("denoise_spatial", "denoise_spatial_display", params, spatial, display, fmt, int(device_ptr), None)

    def denoise_spatial_variance(self, params=None, spatial=None, with_result=False):
        """The luminance variance of every pixel after the estimate, before the first iteration (H x W float32); for inspection."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        r = DenoiseSpatialResult()
        self._feature_call("denoise_spatial", "denoise_spatial_variance", params, spatial, _ptr(out), r)
        return (out, r.as_dict()) if with_result else out

    # -- adaptive sampling (include/hrcore_adaptive.h)
    def set_sample_mask(self, mask):
        """Install a sample mask (H x W, row 0 = bottom like the frame, non-zero = the pixel is sampled by the passes requested from now
        on), or remove it with None.  Completes the enqueued passes first; clear() and resize() remove the mask too."""
        if mask is None:
            self._feature_call("adaptive", "sample_mask_set", None)
            return
        m = np.asarray(mask)
        m = np.ascontiguousarray(m if m.dtype == np.uint8 else m != 0, dtype=np.uint8)  # (bytes go as they are: any non-zero value counts)
        if m.shape != (self.height, self.width):
            raise ValueError(f"sample mask of shape {m.shape} for a frame of {(self.height, self.width)}")
        self._feature_call("adaptive", "sample_mask_set", _ptr(m, u8p))

    def sample_mask(self):
        """(the mask in force as H x W uint8 of 0 / 1, whether one is installed); all ones when there is none."""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        inst = C.c_int32()
        self._feature_call("adaptive", "sample_mask_get", _ptr(out, u8p), C.byref(inst))
        return out, bool(inst.value)

    def adaptive_update(self, params=None, install=True):
        """Estimate every pixel's error from the frame and the MOMENTS plane (set_aovs(HR_AOV_MOMENTS) before the first pass), build the
        sample mask from it and, with install, put it in force.  params: an AdaptiveParams (heatray_amd.adaptive.default_params()),
        None = the defaults.  Returns the AdaptiveResult."""
        r = AdaptiveResult()
        self._feature_call("adaptive", "adaptive_update", params, bool(install), r)
        return r

    def adaptive_error_to_device(self, device_ptr, stream=None):
        """Asynchronous copy of the last adaptive_update's error map (W x H floats) into device memory; ordered like aov_to_device."""
        self._feature_call("adaptive", "adaptive_error_copy", int(device_ptr), stream or 0)

    def adaptive_error(self):
        """The error map of the last adaptive_update as H x W float32 (+inf: fewer than min_samples samples)."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._feature_call("adaptive", "adaptive_error_readback", _ptr(out))
        return out

    # -- history reprojection (include/hrcore_history.h)
    def history_capture(self, pass_params):
        """Turn the frame and the three AOV planes (set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS) before the first pass) into the history, as
        seen by the camera of `pass_params` (view_matrix, fov_tan, aspect_ratio).  The history survives clear()."""
        self._feature_call("history", "history_capture", pass_params)

    def history_merge(self, pass_params, params=None):
        """Add the captured history to the frame and the planes of the view being rendered with `pass_params`; once per clear().  params: a
        HistoryParams (heatray_amd.history.default_params()), None = the defaults.  Returns the HistoryResult as a dict."""
        r = HistoryResult()
        self._feature_call("history", "history_merge", pass_params, params, r)
        return r.as_dict()

    def history_drop(self):
        self._feature_call("history", "history_drop")

    def history_info(self):
        """(is there a captured history, the complete passes of the frame it was captured from)"""
        have, n = C.c_int32(), C.c_uint32()
        self._feature_call("history", "history_info", C.byref(have), C.byref(n))
        return bool(have.value), int(n.value)

    def history(self):
        """The captured history as 3 x H x W x 4 float32: H0 (mean colour, samples), H1 (mean second moment, coverage), H2 (unit normal,
        mean depth; +inf: sky)."""
        out = np.empty((3, self.height, self.width, 4), dtype=np.float32)
        self._feature_call("history", "history_readback", _ptr(out))
        return out

    # -- progressive merge and preview (include/hrcore_reproject.h)
    def reproject_merge(self, pass_params, params=None):
        """history_merge's progressive form: the sampled pixels no earlier call has examined since clear() take over their history; any
        number of calls per clear().  params: a HistoryParams, None = the defaults.  Returns the ReprojectResult as a dict."""
        r = ReprojectResult()
        self._feature_call("reproject", "reproject_merge", pass_params, params, r)
        return r.as_dict()

    def reproject_examined(self):
        """The examined bits as H x W bool (row 0 = bottom like the frame)."""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        self._feature_call("reproject", "reproject_examined_get", _ptr(out, u8p))
        return out.astype(bool)

    def reproject_preview(self, pass_params, params=None):
        """(H x W x 4 float32, the ReprojectPreviewResult as a dict): every sampled pixel's own mean and, in the pixels without a sample,
        the history behind a neighbour's guide (alpha 1) or 0 0 0 0.  Changes nothing."""
        p = f32p()
        w, h = C.c_int32(), C.c_int32()
        r = ReprojectPreviewResult()
        self._feature_call("reproject", "reproject_preview_readback", pass_params, params, C.byref(p), C.byref(w), C.byref(h), r)
        return _image(p, w, h), r.as_dict()

    def reproject_preview_to_device(self, device_ptr, pass_params, params=None, stream=None):
        """Asynchronous: the preview (W x H float4) into device memory, e.g. a torch tensor; ordered like denoise_to_device."""
        self._feature_call("reproject", "reproject_preview", pass_params, params, int(device_ptr), stream or 0, None)

    # -- auto-exposure (include/hrcore_exposure.h)
    def exposure_meter(self, params=None, image=None):
        """Meters the frame (completing the enqueued passes), or `image`: the device pointer of a W x H float4 image in accumulation
        format, e.g. a torch tensor that denoise_to_device filled.  params: an ExposureParams (heatray_amd.exposure.default_params()),
        None = the defaults.  Returns the ExposureResult as a dict."""
        r = ExposureResult()
        self._feature_call("exposure", "exposure_meter", params, int(image) if image else 0, r)
        return r.as_dict()

    def exposure_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None, image=None):
        """Asynchronous: meters like exposure_meter and resolves the metered image, at the metered scale, into device memory (like
        display_device; fmt may carry HR_DISPLAY_PROGRESSIVE).  Returns the passes shown (0 for an `image`)."""
        display = display if display is not None else display_params()
        shown = C.c_uint32()
        self._feature_call("exposure", "exposure_display", params, display, fmt, int(image) if image else 0, int(device_ptr), C.byref(shown))
        return int(shown.value)

    def exposure_last(self, with_bins=False):
        """The last metering's ExposureResult as a dict (waits for it); with_bins: (the dict, its 256 bins as uint64)."""
        r = ExposureResult()
        bins = np.zeros(HR_EXPOSURE_BINS, np.uint64)
        self._feature_call("exposure", "exposure_last", r, _ptr(bins, u64p) if with_bins else None)
        return (r.as_dict(), bins) if with_bins else r.as_dict()

    def exposure_reset(self):
        """Forgets the adaptation state: the next metering's scale is its target."""
        self._feature_call("exposure", "exposure_reset")

    # -- the convergence metric (include/hrcore_metric.h)
    def metric_compare(self, reference, image=None, params=None):
        """The relative L2 distance of the frame (completing the enqueued passes), or of `image`, from `reference`: device pointers of
        W x H float4 images in accumulation format, e.g. a torch tensor holding a kept copy of a converged frame.  params: a MetricParams
        (heatray_amd.metric.default_params()), None = the whole image.  Waits; returns the MetricResult as a dict (`value` is the metric)."""
        r = MetricResult()
        self._feature_call("metric", "metric_compare", params, int(image) if image else 0, int(reference) if reference else 0, r)
        return r.as_dict()

    def metric_estimate(self, params=None):
        """The relative L2 distance the frame's sample moments predict between its luminance image and its own limit (HR_AOV_MOMENTS must
        be enabled before the frame's first pass).  Waits; returns the MetricResult as a dict."""
        r = MetricResult()
        self._feature_call("metric", "metric_estimate", params, r)
        return r.as_dict()

    def metric_last(self, with_bins=False):
        """The last measurement's MetricResult as a dict; with_bins: (the dict, the 256 bins of num, those of den, as uint64)."""
        r = MetricResult()
        num, den = np.zeros(HR_METRIC_BINS, np.uint64), np.zeros(HR_METRIC_BINS, np.uint64)
        self._feature_call("metric", "metric_last", r, _ptr(num, u64p) if with_bins else None, _ptr(den, u64p) if with_bins else None)
        return (r.as_dict(), num, den) if with_bins else r.as_dict()

    # -- firefly suppression (include/hrcore_despeckle.h)
    def despeckle(self, params=None, with_moments=False, with_result=False):
        """The despeckled frame (H x W x 4 float32, accumulation format like readback()) of the passes rendered so far; needs
        HR_AOV_MOMENTS enabled before the frame's first pass.  params: a DespeckleParams (heatray_amd.despeckle.default_params()),
        None = the defaults.  with_moments: and the despeckled MOMENTS plane; with_result: and the DespeckleResult as a dict; the image
        alone, or a tuple in that order."""
        p, m = f32p(), f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle_readback", params, C.byref(p), C.byref(m) if with_moments else None,
                           C.byref(w), C.byref(h), C.byref(n), r)
        out = [_image(p, w, h)]
        if with_moments:
            out.append(_image(m, w, h))
        if with_result:
            out.append(r.as_dict())
        return out[0] if len(out) == 1 else tuple(out)

    def despeckle_to_device(self, out_ptr, moments_out_ptr=None, params=None, frame=None, moments=None, stream=None, with_result=False):
        """Asynchronous: the despeckled frame, and with moments_out_ptr the despeckled moments, (W x H float4 each) into device memory,
        e.g. torch tensors; ordered like denoise_to_device.  frame / moments: device pointers of a caller's pair instead of the
        context's own (both or neither).  with_result: waits and returns the DespeckleResult as a dict."""
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle", params, int(frame) if frame else 0, int(moments) if moments else 0, int(out_ptr) if out_ptr else 0,
                           int(moments_out_ptr) if moments_out_ptr else 0, stream or 0, None, r if with_result else None)
        return r.as_dict() if with_result else None

    def despeckle_denoise(self, params=None, dparams=None, spatial=False, sparams=None, with_result=False):
        """denoise() (spatial: denoise_spatial()) run from the despeckled frame and moments instead of the raw ones.  params: a
        DespeckleParams, dparams: a DenoiseParams, sparams: a DenoiseSpatialParams; None = the defaults.  with_result: (image, the
        DespeckleResult as a dict)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle_denoise_readback", params, dparams, bool(spatial), sparams, C.byref(p), C.byref(w), C.byref(h), C.byref(n), r)
        img = _image(p, w, h)
        return (img, r.as_dict()) if with_result else img

    def despeckle_denoise_to_device(self, device_ptr, params=None, dparams=None, spatial=False, sparams=None, stream=None):
        """Asynchronous: despeckle_denoise's image (W x H float4) into device memory; ordered like denoise_to_device."""
        self._feature_call("despeckle", "despeckle_denoise", params, dparams, bool(spatial), sparams, int(device_ptr) if device_ptr else 0, stream or 0, None, None)

    # -- mesh preparation (include/hrcore_mesh.h)
    def prepare_mesh(self, positions, indices, uvs=None, normals=None, mode=HR_TRIANGLES, params=None, with_result=False):
        """(normals, tangents, bitangents) of a mesh that comes without them, V x 3 float32 each, None for what params.want does not ask
        for.  positions: V x 3, indices: the index list of `mode`; uvs (V x 2) are needed for tangents, normals (V x 3) for tangents
        without normals.  Strided arrays go as they are (the last axis contiguous).  params: a MeshParams
        (heatray_amd.meshprep.default_params()), None = the defaults.  with_result: and the MeshResult as a dict.  A side call: the scene
        and the frame are left alone."""
        pos, ps = _strided(positions, 3)
        uv, us = _strided(uvs, 2)
        nrm, ns = _strided(normals, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        want = params.want if params is not None else HR_MESH_WANT_NORMALS
        d = MeshDesc()
        d.positions, d.uvs, d.normals = _ptr(pos), _ptr(uv), _ptr(nrm)
        d.position_stride, d.uv_stride, d.normal_stride = ps, us, ns
        d.n_vertices = pos.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        out = [np.empty((pos.shape[0], 3), dtype=np.float32) if want & bit else None
               for bit in (HR_MESH_WANT_NORMALS, HR_MESH_WANT_TANGENTS, HR_MESH_WANT_TANGENTS)]
        r = MeshResult()
        self._feature_call("mesh", "mesh_prepare", d, params, *(_ptr(a) for a in out), r)
        return (*out, r.as_dict()) if with_result else tuple(out)

    def add_mesh_prepared(self, positions, indices, uvs=None, **add_mesh_kwargs):
        """add_mesh for a mesh without normals: prepare_mesh makes them, and with uvs the tangents and bitangents too (weight ANGLE,
        weld on); the remaining keywords are add_mesh's (mode included).  Returns the geometry id."""
        p = MeshParams(HR_MESH_WEIGHT_ANGLE, 1, HR_MESH_WANT_NORMALS | (HR_MESH_WANT_TANGENTS if uvs is not None else 0))
        n, t, b = self.prepare_mesh(positions, indices, uvs=uvs, mode=add_mesh_kwargs.get("mode", HR_TRIANGLES), params=p)
        return self.add_mesh(positions, n, indices, uvs=uvs, tangents=t, bitangents=b, **add_mesh_kwargs)

    def mesh_last(self):
        """The last successful prepare_mesh's MeshResult as a dict."""
        r = MeshResult()
        self._feature_call("mesh", "mesh_last", r)
        return r.as_dict()

    # -- deformable meshes (include/hrcore_deform.h)
    def update_mesh(self, gid, positions, normals=None, uvs=None, tangents=None, bitangents=None, colors=None, params=None, with_result=False):
        """New vertex data for mesh `gid`, in its device block: positions (V x 3) and whichever other attributes are given; None leaves
        an attribute as it is.  Strided arrays go as they are (the last axis contiguous).  params: a DeformParams
        (heatray_amd.deform.params(regenerate=...)), None = the defaults.  The scene needs a commit afterwards: it refits.
        with_result: the DeformResult as a dict."""
        arrays = [_strided(a, comps) for a, comps in zip((positions, normals, uvs, tangents, bitangents, colors), (3, 3, 2, 3, 3, 3))]
        d = MeshDesc()
        d.positions, d.normals, d.uvs, d.tangents, d.bitangents, d.colors = (_ptr(a) for a, _ in arrays)
        d.position_stride, d.normal_stride, d.uv_stride, d.tangent_stride, d.bitangent_stride, d.color_stride = (s for _, s in arrays)
        d.n_vertices = arrays[0][0].shape[0]
        r = DeformResult()
        self._feature_call("deform", "geom_update", gid, d, params, r)
        self._mesh_vertices[gid] = d.n_vertices
        return r.as_dict() if with_result else None

    def mesh_attribute(self, gid, attribute, n_vertices=None):
        """Attribute HR_GEOM_* of mesh `gid` as the device block holds it: V x 3 float32 (V x 2 for uvs).  The C call does not say how
        many vertices the mesh has: add_mesh, add_mesh_strided and update_mesh remember it; n_vertices names it for any other mesh."""
        V = n_vertices if n_vertices is not None else self._mesh_vertices.get(gid)
        if V is None:
            # (an id this engine does not know: the library names the cause, if the call fails; else the count is missing)
            self._feature_call("deform", "geom_get_attribute", gid, attribute, None)
            raise ValueError(f"mesh_attribute: give n_vertices for mesh {gid}")
        out = np.empty((V, 2 if attribute == HR_GEOM_UVS else 3), dtype=np.float32)
        self._feature_call("deform", "geom_get_attribute", gid, attribute, _ptr(out))
        return out

    def deform_bind(self, gid, morph_positions=None, morph_normals=None, joints=None, weights=None, n_joints=None):
        """The mesh as it stands becomes the rest pose of a rig: morph_positions / morph_normals K x V x 3 deltas, joints V x 4 indices
        and weights V x 4; n_joints: the rig's joint count, None = the highest index named + 1.  A second bind replaces the first."""
        mp = None if morph_positions is None else _f32(morph_positions)
        mn = None if morph_normals is None else _f32(morph_normals)
        j = None if joints is None else np.ascontiguousarray(joints, dtype=np.uint32)
        w = None if weights is None else _f32(weights)
        rig = DeformRig()
        rig.morph_positions, rig.morph_normals, rig.joints, rig.weights = _ptr(mp), _ptr(mn), _ptr(j, u32p), _ptr(w)
        rig.n_morph = 0 if mp is None else mp.reshape(-1, *mp.shape[-2:]).shape[0]
        if n_joints is None:
            n_joints = 0 if j is None or not j.size else int(j.max()) + 1
        rig.n_joints = n_joints
        self._feature_call("deform", "deform_bind", gid, rig)
        self._deform_rigs[gid] = (rig.n_morph, rig.n_joints)

    def deform_pose(self, gid, morph_weights=None, joint_matrices=None, params=None, with_result=False):
        """Pose the bound mesh `gid` on the device: morph_weights K floats, joint_matrices J x 4 x 4 (numpy's m[row][col]; the ABI's
        column-major order is made here).  params as update_mesh's.  The scene needs a commit afterwards."""
        mw = None if morph_weights is None else _f32(morph_weights).reshape(-1)
        jm = None if joint_matrices is None else _f32(np.transpose(_f32(joint_matrices).reshape(-1, 4, 4), (0, 2, 1)))
        K, J = self._deform_rigs.get(gid, (0, 0))  # (the library reads as many as the rig has)
        if (mw is not None and mw.size < K) or (jm is not None and jm.shape[0] < J):
            raise ValueError(f"deform_pose: mesh {gid} is bound to {K} morphs and {J} joints")
        r = DeformResult()
        self._feature_call("deform", "deform_pose", gid, _ptr(mw), _ptr(jm), params, r)
        return r.as_dict() if with_result else None

    def deform_unbind(self, gid):
        self._feature_call("deform", "deform_unbind", gid)
        self._deform_rigs.pop(gid, None)

    def deform_last(self):
        """The last successful update_mesh's or deform_pose's DeformResult as a dict."""
        r = DeformResult()
        self._feature_call("deform", "deform_last", r)
        return r.as_dict()

    # -- ray queries (include/hrcore_query.h)
    @staticmethod
    def _query_desc(n, origins, dirs, tmax, skip, strides, any_hit, tmin, hits, surfaces):
        d = QueryDesc()
        d.n, d.flags = int(n), HR_QUERY_ANY_HIT if any_hit else 0
        d.origins, d.directions, d.tmax, d.skip_prim = origins or None, dirs or None, tmax or None, skip or None
        d.origin_stride, d.direction_stride, d.tmax_stride, d.skip_stride = (int(v) for v in strides)
        d.tmin = -1.0 if tmin is None else float(tmin)
        d.hits, d.surfaces = hits or None, surfaces or None
        return d

    def query(self, origins, dirs, tmax=None, skip_prim=None, any_hit=False, surface=False, tmin=None):
        """Trace the caller's rays (numpy, n x 3 each) against the committed scene: the hits (HIT_DTYPE, as debug_trace reports them;
        prim = HR_QUERY_INVALID_RAY for a ray that is not finite), or (hits, surfaces) with surface=True (SURFACE_DTYPE: which mesh, which
        triangle of it, where on it).  any_hit: an occlusion query (prim 0 blocked / -1 clear).  tmin=None: the scene's ray epsilon.
        A float32 array whose rows are strided (a view into an interleaved buffer) goes to the library as it is, stride included."""
        def rows(a, comps, dtype):
            a = np.asarray(a)
            shaped = a.ndim == 2 and a.shape[1] == comps and a.strides[1] == 4 if comps > 1 else a.ndim == 1
            if a.dtype != dtype or not shaped or a.strides[0] % 4 or a.strides[0] < comps * 4:
                a = np.ascontiguousarray(a, dtype=dtype).reshape((-1, comps) if comps > 1 else (-1,))
            return a
        o, d = rows(origins, 3, np.float32), rows(dirs, 3, np.float32)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError(f"query: {n} origins but {d.shape[0]} directions")
        tm = None if tmax is None else rows(tmax, 1, np.float32)
        sk = None if skip_prim is None else rows(skip_prim, 1, np.int32)
        for name, a in (("tmax", tm), ("skip_prim", sk)):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"query: {n} rays but {a.shape[0]} entries of {name}")
        hits = np.empty(n, dtype=HIT_DTYPE)
        surf = np.empty(n, dtype=SURFACE_DTYPE) if surface else None
        addr = lambda a: None if a is None else a.ctypes.data
        stride = lambda a: 0 if a is None or a.shape[0] < 2 else a.strides[0]
        desc = self._query_desc(n, addr(o), addr(d), addr(tm), addr(sk), (stride(o), stride(d), stride(tm), stride(sk)), any_hit, tmin, addr(hits), addr(surf))
        nothing = C.c_float()
        if n == 0:  # (an empty array's address may be null, which the library would call "null origins"; with n = 0 nothing is read or written)
            desc.origins = desc.directions = desc.hits = C.addressof(nothing)
        self._feature_call("query", "query_trace_host", desc)
        return (hits, surf) if surface else hits

    def query_to_device(self, n, origins_ptr, dirs_ptr, hits_ptr=None, surfaces_ptr=None, tmax_ptr=None, skip_ptr=None, strides=(0, 0, 0, 0),
                        any_hit=False, tmin=None, stream=None):
        """Asynchronous: n rays in device memory (raw device pointers, e.g. torch tensors' data_ptr(); strides in bytes for origins,
        directions, tmax, skip_prim, 0 = tight) -> n hr_hit at hits_ptr and / or n hr_query_surface at surfaces_ptr, on `stream` (None: the
        context's).  Ordered behind the last commit; the next commit waits for it (include/hrcore_query.h, ORDERING)."""
        desc = self._query_desc(n, origins_ptr, dirs_ptr, tmax_ptr, skip_ptr, strides, any_hit, tmin, hits_ptr, surfaces_ptr)
        self._feature_call("query", "query_trace", desc, stream or 0)

    def query_pixels(self, pass_params, xy, surface=True, rays=False):
        """The camera rays through the points xy (n x 2, pixel units: the centre of pixel x, y is x + 0.5, y + 0.5, row 0 at the bottom) of
        the frame, traced with tmin = 0: hits, then surfaces with surface=True, then the rays (n x 6: o, d) with rays=True.  hits["t"] is
        the focus_distance that focuses the lens on what the pixel shows."""
        p = _f32(xy).reshape(-1, 2)
        n = p.shape[0]
        hits = np.empty(n, dtype=HIT_DTYPE)
        surf = np.empty(n, dtype=SURFACE_DTYPE) if surface else None
        ro = np.empty((n, 6), dtype=np.float32) if rays else None
        # (an empty array's address may be null: with n = 0 the library gets something to point at, and reads and writes nothing)
        self._feature_call("query", "query_pixels", pass_params, n, _ptr(p) if n else C.pointer(C.c_float()), _ptr(hits, P(Hit)) if n else Hit(),
                           _ptr(surf, P(QuerySurface)), _ptr(ro))
        out = (hits,) + ((surf,) if surface else ()) + ((ro,) if rays else ())
        return out if len(out) > 1 else hits

    def query_last(self):
        """{"rays", "hits", "invalid"} of the last successful query; completes the queries in flight."""
        r = QueryResult()
        self._feature_call("query", "query_last", r)
        return r.as_dict()

    # -- motion reprojection (include/hrcore_motion.h)
    def motion_snapshot(self):
        """Remember the committed pose: every triangle's world-space (p0, e1, e2) and the table of meshes.  Survives clear(), commits
        and resize(); a second snapshot replaces it."""
        self._feature_call("motion", "motion_snapshot")

    def motion_trace(self, pass_params):
        """One pixel-centre ray per pixel of the camera of `pass_params` against the committed scene: where was each pixel's surface
        point in the snapshot's pose?  Writes the motion planes (motion_planes()); returns {"surface_pixels", "sky_pixels",
        "unmatched_pixels"}."""
        r = MotionTraceResult()
        self._feature_call("motion", "motion_trace", pass_params, r)
        return r.as_dict()

    def motion_merge(self, pass_params, params=None):
        """history_merge, gathering where the snapshot says each pixel's surface point was; once per clear(), instead of history_merge or
        reproject_merge.  params: a HistoryParams (heatray_amd.motion.default_params()), None = those defaults.  Returns the
        MotionResult as a dict: history_merge's keys and motion_trace's."""
        r = MotionResult()
        self._feature_call("motion", "motion_merge", pass_params, params, r)
        return r.as_dict()

    def motion_planes(self):
        """The motion planes of the last trace as 2 x H x W x 4 float32: Mv0 (the surface point in the previous pose, 1 / the hit point,
        -1 / 0 0 0 0 for sky), Mv1 (the previous pose's geometric normal, depth; +inf: sky)."""
        out = np.empty((2, self.height, self.width, 4), dtype=np.float32)
        self._feature_call("motion", "motion_readback", _ptr(out))
        return out

    def motion_vectors(self, old_pass_params=None):
        """The screen-space motion of every pixel as H x W x 4 float32: (dx, dy, the point's depth in the old camera, Mv0.w), from the
        planes of the last trace.  old_pass_params None: the captured history's camera."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._feature_call("motion", "motion_vectors_readback", old_pass_params, _ptr(out))
        return out

    def motion_vectors_to_device(self, device_ptr, old_pass_params=None, stream=None):
        """Asynchronous: the same image into device memory (a raw pointer, 16-byte aligned) on `stream` (None: the context's)."""
        self._feature_call("motion", "motion_vectors", old_pass_params, C.cast(device_ptr, f32p), stream or 0)

    def motion_snapshot_triangles(self):
        """The snapshot as T x 12 float32 in submission order: p0.xyz e1.xyz e2.xyz 0 0 0."""
        out = np.empty((self.motion_info()["triangles"], 12), dtype=np.float32)
        self._feature_call("motion", "motion_snapshot_readback", _ptr(out) if out.size else C.pointer(C.c_float()))
        return out

    def motion_drop(self):
        self._feature_call("motion", "motion_drop")

    def motion_info(self):
        """{"snapshot", "traced", "triangles", "meshes", "bytes"}"""
        r = MotionInfo()
        self._feature_call("motion", "motion_info", r)
        return r.as_dict()

    def debug_trace(self, origins, dirs, tmax=None, skip_prim=None, any_hit=False):
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = o.shape[0]
        tm = None if tmax is None else _f32(tmax).reshape(-1)
        sk = None if skip_prim is None else np.ascontiguousarray(skip_prim, dtype=np.int32).reshape(-1)
        out = np.empty(n, dtype=HIT_DTYPE)
        self._call("debug_trace", n, _ptr(o), _ptr(d), _ptr(tm), _ptr(sk, i32p), int(any_hit), _ptr(out, P(Hit)))
        return out


class GroupEngine(Engine):
    """An Engine whose handle is a context group (include/hrcore_group.h): member i renders the tiles t % n == i on
    device_ids[i]; every Engine call works on it, plus the group's own two."""

    def __init__(self, lib, device_ids=None, tile_size=32, stream=None, flags=0, memory_budget=0):
        self._init(lib, "hr_")
        missing = [s for s in GROUP_SYMBOLS if s not in self._fns]
        if missing:
            raise EngineError(f"the loaded libhrcore has no context groups (lacks {missing}): rebuild it")
        self._check_version("abi_version", HR_ABI_VERSION)
        self._check_version("group_api_version", HR_GROUP_API_VERSION)
        ids = None if device_ids is None else (C.c_int32 * max(1, len(device_ids)))(*device_ids)
        n = 0 if device_ids is None else len(device_ids)
        desc = CtxDesc(0, 0, 1, tile_size, stream, flags, int(memory_budget))
        rc = self._fn("ctx_create_group")(desc, ids, n, C.byref(self._ctx))
        if rc != HR_OK:
            self._ctx = C.c_void_p()
            raise EngineError(f"hr_ctx_create_group({list(device_ids) if device_ids is not None else 'every device'}) failed with status {rc} "
                              "(no usable HIP device, a bad device id or more than 16 members?)")

    def group_info(self):
        """{"n_members", "device_ids", "owned_pixels"} of the group."""
        g = GroupInfo()
        self._call("group_get_info", g)
        n = g.n_members
        return {"n_members": n, "device_ids": list(g.device_ids[:n]), "owned_pixels": list(g.owned_pixels[:n])}

    def member_stats(self, member, kernel_times=False):
        """PassStats of one member (completes its passes first); with kernel_times, (stats, KernelTimes)."""
        s, t = PassStats(), KernelTimes()
        self._call("group_member_stats", member, s, t if kernel_times else None)
        return (s, t) if kernel_times else s
