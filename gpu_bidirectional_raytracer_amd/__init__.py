"""MI355X-native bidirectional path tracer: the render path of sim186/gpu_bidirectional_raytracer
(per-pixel eye path with NEE + VLP connection, MT607 random table, light pass) as hand-written
HIP kernels for gfx950 behind a C-ABI (include/bdpt.h, libbdpt.so).

This package is the host-side mirror of the reference's operator interface (src/smallpt_cpu.c,
src/display_func.c): `SmallPT` keeps the reference's names (AllocateBuffers, UpdateRendering,
UpdateRendering2, ReInit, ReInitScene, SavePPM, KeyFunc, SpecialFunc) and argument meaning;
`Renderer` is a thin object over one C-ABI context.  No torch types anywhere: torch is only
used by bench.py for torch.distributed plumbing.
"""
from __future__ import annotations

import ctypes
import os
import struct
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import (BDPT_OK, CHOICES, COUNTER_CAP, DEFAULT_DAT, DIFF, FEATURES, KEY_DOWN, KEY_LEFT, KEY_PAGE_DOWN,
                   KEY_PAGE_UP, KEY_RIGHT, KEY_UP, LIGHT_POINTS, LITE, RAND_N, REFR, SCENE_DIR, SPEC,
                   CHAIN_BRANCHES, CHAIN_KIND_DIFFUSE, CHAIN_KIND_EMITTER, CHAIN_KIND_EXHAUSTED, CHAIN_KIND_MISS, ChainBuffers,
                   DENOISE_MATERIALS, AovBuffers, BdptError, Camera, DenoiseNoiseParams, DenoiseParams, LightPath, NoiseParams, NoiseSummary, PassState, PreviewParams,
                   RandState, ReprojectParams, Sphere, Vec, lib)

__all__ = [
    "Vec", "Sphere", "Camera", "LightPath", "Renderer", "SmallPT", "PassScheduler", "read_scene",
    "default_scene", "update_camera", "camera_key", "sphere_key", "save_ppm", "ppm_name", "glibc_rand",
    "spheres_to_array", "RAND_N", "LIGHT_POINTS", "COUNTER_CAP", "DIFF", "SPEC", "REFR", "LITE",
    "SCENE_DIR", "DEFAULT_DAT", "BdptError", "AOV_PLANES", "CHAIN_PLANES", "CHAIN_KIND_DIFFUSE",
    "CHAIN_KIND_EMITTER", "CHAIN_KIND_MISS", "CHAIN_KIND_EXHAUSTED",
]

SPHERE_DTYPE = np.dtype([("rad", "<f4"), ("p", "<f4", 3), ("e", "<f4", 3), ("c", "<f4", 3),
                         ("refl", "<i4")])
assert SPHERE_DTYPE.itemsize == ctypes.sizeof(Sphere)
LIGHTPATH_DTYPE = np.dtype([("hp", "<f4", 3), ("rad", "<f4", 3), ("nl", "<f4", 3)])


AOV_PLANES = ("id", "t", "dp", "position", "normal", "dir")     # bdpt_aov_buffers, in its order
CHAIN_PLANES = ("id", "first_id", "kind", "bounces", "t", "dp", "position", "normal", "dir",
                "throughput")                                      # bdpt_chain_buffers, in its order


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def spheres_to_array(spheres) -> np.ndarray:
    """ctypes Sphere array / list of Sphere / structured array -> contiguous SPHERE_DTYPE array."""
    if isinstance(spheres, np.ndarray):
        return np.ascontiguousarray(spheres.astype(SPHERE_DTYPE, copy=False))
    n = len(spheres)
    arr = np.zeros(n, SPHERE_DTYPE)
    if n:
        buf = (Sphere * n)(*spheres)
        ctypes.memmove(arr.ctypes.data, buf, ctypes.sizeof(buf))
    return arr


def _sphere_ptr(arr: np.ndarray):
    return ctypes.cast(ctypes.c_void_p(arr.ctypes.data), ctypes.POINTER(Sphere))


# ---- host utilities (display_func.c / smallpt_cpu.c) ----------------------------------------

def read_scene(path: str) -> Tuple[Camera, np.ndarray]:
    """ReadScene (display_func.c:112-175): returns (camera with orig/target set, spheres)."""
    cam = Camera()
    sp = ctypes.POINTER(Sphere)()
    n = ctypes.c_uint(0)
    rc = lib.bdpt_read_scene(os.fsencode(path), ctypes.byref(cam), ctypes.byref(sp), ctypes.byref(n))
    if rc != BDPT_OK:
        raise BdptError(rc, f"cannot read scene {path}")
    arr = np.zeros(n.value, SPHERE_DTYPE)
    if n.value:
        ctypes.memmove(arr.ctypes.data, sp, n.value * ctypes.sizeof(Sphere))
    lib.bdpt_free_scene(sp)
    return cam, arr


def default_scene() -> Tuple[Camera, np.ndarray]:
    """CornellSpheres (scene.h:7-18) + the no-argument camera (smallpt_cpu.c:404-405)."""
    cam = Camera()
    buf = (Sphere * 9)()
    n = lib.bdpt_default_scene(ctypes.byref(cam), buf)
    arr = np.zeros(n, SPHERE_DTYPE)
    ctypes.memmove(arr.ctypes.data, buf, ctypes.sizeof(buf))
    return cam, arr


def update_camera(cam: Camera, width: int, height: int) -> Camera:
    """UpdateCamera (display_func.c:177-190); width/height are the internal (+1) sizes."""
    lib.bdpt_update_camera(ctypes.byref(cam), int(width), int(height))
    return cam


_KEYS = {"up": KEY_UP, "down": KEY_DOWN, "left": KEY_LEFT, "right": KEY_RIGHT,
         "page_up": KEY_PAGE_UP, "page_down": KEY_PAGE_DOWN}


def camera_key(cam: Camera, key) -> bool:
    """KeyFunc/SpecialFunc camera moves; returns True when the key moved the camera."""
    code = _KEYS[key] if isinstance(key, str) and len(key) > 1 else (ord(key) if isinstance(key, str) else int(key))
    return bool(lib.bdpt_camera_key(ctypes.byref(cam), code))


def sphere_key(spheres: np.ndarray, current: int, key: str) -> bool:
    """KeyFunc sphere edits ('4','6','8','2','9','3'), in place; True when a sphere moved."""
    assert spheres.dtype == SPHERE_DTYPE and spheres.flags.c_contiguous
    return bool(lib.bdpt_sphere_key(_sphere_ptr(spheres), len(spheres), int(current), ord(key)))


def save_ppm(path: str, rgba: np.ndarray, binary: bool = False) -> None:
    """SavePPM (smallpt_cpu.c:239-262): ASCII P3, rows bottom-up; binary=True writes P6."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    fn = lib.bdpt_save_ppm_binary if binary else lib.bdpt_save_ppm
    rc = fn(os.fsencode(path), _ptr(rgba), w, h)
    if rc != BDPT_OK:
        raise BdptError(rc, f"cannot write {path}")


def ppm_name(total_time: float, current_sample: int) -> str:
    """SavePPM's file name (smallpt_cpu.c:245): max1_secondi<total_time %.3f>_exe<sample>.ppm."""
    buf = ctypes.create_string_buffer(128)
    lib.bdpt_ppm_name(buf, len(buf), float(total_time), int(current_sample))
    return buf.value.decode()


def glibc_rand(n: int, seed: int = 1) -> np.ndarray:
    """n values of glibc rand() after srand(seed) (the library's own implementation)."""
    st = RandState()
    lib.bdpt_srand(ctypes.byref(st), seed)
    return np.array([lib.bdpt_rand(ctypes.byref(st)) for _ in range(n)], dtype=np.int64)


class PassScheduler:
    """sid = rand() % RAND_N and the flag/vlp_index state machine of smallpt_cpu.c:270,292-293."""

    def __init__(self):
        self.state = PassState()
        lib.bdpt_pass_state_init(ctypes.byref(self.state))

    def light(self) -> None:
        lib.bdpt_pass_state_light(ctypes.byref(self.state))

    def next(self, npass: int) -> Tuple[np.ndarray, np.ndarray]:
        sid = np.empty(npass, np.uint32)
        vlp = np.empty(npass, np.int32)
        if npass:
            lib.bdpt_pass_schedule(ctypes.byref(self.state), npass, _ptr(sid), _ptr(vlp))
        return sid, vlp

    @property
    def flag(self) -> int:
        return self.state.flag

    @property
    def vlp_index(self) -> int:
        return self.state.vlp_index


# ---- one render context on one GPU -----------------------------------------------------------

class Renderer:
    """One C-ABI context (bdpt_create): device buffers, MT table, VLPs and the accumulation."""

    def __init__(self, spheres, width: int, height: int, camera: Optional[Camera] = None,
                 dat_path: str = DEFAULT_DAT, device: int = 0, devices: Optional[Sequence[int]] = None):
        """devices=[d0, d1, ...]: one multi-device context (bdpt_create_multi): pixel bands over
        the devices, frame assembled on d0 (RCCL when the devices are distinct)."""
        self.width, self.height = int(width), int(height)
        self.spheres = spheres_to_array(spheres)
        h = ctypes.c_void_p()
        if devices is not None:
            devs = np.ascontiguousarray(devices, dtype=np.int32)
            rc = lib.bdpt_create_multi(ctypes.byref(h), _sphere_ptr(self.spheres), len(self.spheres),
                                       self.width, self.height, os.fsencode(dat_path), _ptr(devs), len(devs))
        else:
            rc = lib.bdpt_create(ctypes.byref(h), _sphere_ptr(self.spheres), len(self.spheres),
                                 self.width, self.height, os.fsencode(dat_path), int(device))
        if rc != BDPT_OK:
            raise BdptError(rc, lib.bdpt_create_error().decode())
        self._h = h
        if camera is not None:
            self.set_camera(camera)

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            lib.bdpt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc: int) -> None:
        if rc != BDPT_OK:
            raise BdptError(rc, lib.bdpt_last_error(self._h).decode())

    # -- state
    def set_camera(self, cam: Camera) -> None:
        self.camera = cam
        self._chk(lib.bdpt_set_camera(self._h, ctypes.byref(cam)))

    def set_scene(self, spheres) -> None:
        self.spheres = spheres_to_array(spheres)
        self._chk(lib.bdpt_set_scene(self._h, _sphere_ptr(self.spheres), len(self.spheres)))

    def reset_accum(self) -> None:
        self._chk(lib.bdpt_reset_accum(self._h))

    def set_shard(self, shard: int, nshards: int, band_rows: int = 8) -> None:
        self._chk(lib.bdpt_set_shard(self._h, shard, nshards, band_rows))

    def set_streams(self, streams: int) -> None:
        """Pass streams per pixel (0 = auto: measured choice, -1 = one pass per lane, 1 = fused); results are bit-identical for every value."""
        self._chk(lib.bdpt_set_streams(self._h, streams))

    @property
    def last_streams(self) -> int:
        return int(lib.bdpt_last_streams(self._h))

    @property
    def stream_choice(self) -> int:
        """BDPT_CHOICE_* bits of the auto stream mode's decision (0 while measuring / not auto)."""
        return int(lib.bdpt_stream_choice(self._h))

    def set_stream_choice(self, choice: int) -> None:
        """Apply a decision of the auto stream mode (e.g. rank 0's) without measuring."""
        self._chk(lib.bdpt_set_stream_choice(self._h, int(choice)))

    def device_mode(self, k: int = 0) -> dict:
        """Device k's last kernel: {streams, features, choice} (bdpt_device_mode)."""
        st, ft, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._chk(lib.bdpt_device_mode(self._h, k, ctypes.byref(st), ctypes.byref(ft), ctypes.byref(ch)))
        return {"streams": st.value, "features": [n for b, n in sorted(FEATURES.items()) if ft.value & b],
                "choice": [n for b, n in sorted(CHOICES.items()) if ch.value & b]}

    def set_specialize(self, on: bool) -> None:
        """Scene-specialised kernels (run-time compiled, <= 64 spheres); results are bit-identical."""
        self._chk(lib.bdpt_set_specialize(self._h, int(bool(on))))

    @property
    def last_specialized(self) -> bool:
        return bool(lib.bdpt_last_specialized(self._h))

    @property
    def specialize_status(self) -> str:
        """Why the last path pass did not run a specialised kernel ('' if it did or was not asked)."""
        return lib.bdpt_specialize_status(self._h).decode()

    def set_traversal(self, mode: str) -> None:
        """'auto' (BVH when the scene has one), 'brute' (every sphere) or 'bvh'."""
        self._chk(lib.bdpt_set_traversal(self._h, {"auto": 0, "brute": 1, "bvh": 2}[mode]))

    @property
    def has_bvh(self) -> bool:
        return bool(lib.bdpt_scene_has_bvh(self._h))

    @property
    def last_traversal(self) -> str:
        return {1: "brute", 2: "bvh"}[int(lib.bdpt_last_traversal(self._h))]

    @property
    def last_features(self) -> list:
        """What the last path-pass kernel compiled in (include/bdpt.h BDPT_FEAT_*), by name."""
        bits = int(lib.bdpt_last_kernel_features(self._h))
        return [name for bit, name in sorted(FEATURES.items()) if bits & bit]

    def path_lds(self) -> dict:
        """{static, dynamic, limit} in bytes: the LDS of the last path_passes call's largest launch
        (refused or not) and what the device allows a workgroup (bdpt_path_lds)."""
        st, dy, lim = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
        self._chk(lib.bdpt_path_lds(self._h, ctypes.byref(st), ctypes.byref(dy), ctypes.byref(lim)))
        return {"static": st.value, "dynamic": dy.value, "limit": lim.value}

    @property
    def num_devices(self) -> int:
        return int(lib.bdpt_num_devices(self._h))

    @property
    def reduce_backend(self) -> str:
        """'rccl' / 'peer' for a multi-device context, 'none' for a one-device context."""
        return lib.bdpt_reduce_backend(self._h).decode()

    @property
    def reduce_info(self) -> str:
        """The frame reduce in words (bdpt_reduce_info): RCCL version, ranks and devices, or why not RCCL."""
        buf = ctypes.create_string_buffer(512)
        n = lib.bdpt_reduce_info(self._h, buf, len(buf))
        if n < 0:
            self._chk(n)
        return buf.value.decode()

    def reduce_frame(self) -> None:
        self._chk(lib.bdpt_reduce_frame(self._h))

    # -- work
    def generate_rand(self, seed: int) -> None:
        self._chk(lib.bdpt_generate_rand(self._h, seed))

    def light_pass(self, current_sample: int = 0) -> None:
        self._chk(lib.bdpt_light_pass(self._h, current_sample))

    def path_passes(self, sid: Sequence[int], vlp: Sequence[int], sync: bool = True, tiles=None) -> None:
        """tiles: a [tiles_y, tiles_x] bool or uint8 array over the 32 x 8 tiles of noise_tiles();
        only the pixels of tiles with a non-zero entry are rendered, every other pixel keeps its
        state bit for bit (bdpt_path_passes_tiles).  None: every pixel."""
        sid = np.ascontiguousarray(sid, dtype=np.uint32)
        vlp = np.ascontiguousarray(vlp, dtype=np.int32)
        assert sid.shape == vlp.shape and sid.ndim == 1
        if tiles is None:
            self._chk(lib.bdpt_path_passes(self._h, _ptr(sid), _ptr(vlp), len(sid)))
        else:
            mask = self._tile_mask(tiles)
            self._chk(lib.bdpt_path_passes_tiles(self._h, _ptr(sid), _ptr(vlp), len(sid), _ptr(mask)))
        if sync:
            self.synchronize()

    def _tile_mask(self, tiles) -> np.ndarray:
        """`tiles` as the contiguous uint8 [tiles_y, tiles_x] mask the C-ABI takes (non-zero -> 1)."""
        mask = np.ascontiguousarray(np.asarray(tiles) != 0, dtype=np.uint8)
        ty, tx = -(-self.height // 8), -(-self.width // 32)
        if mask.shape != (ty, tx):
            raise ValueError(f"tiles must have shape {(ty, tx)} (tiles_y, tiles_x), not {mask.shape}")
        return mask

    def synchronize(self) -> None:
        self._chk(lib.bdpt_synchronize(self._h))

    def calls_in_flight(self) -> int:
        """How many path_passes calls the device has not finished (0..4 per device; 0 on the CPU
        backend).  Never waits: it tells whether the next call is queued behind running passes."""
        n = ctypes.c_int()
        self._chk(lib.bdpt_calls_in_flight(self._h, ctypes.byref(n)))
        return n.value

    def last_path_ms(self) -> float:
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_path_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def path_timing(self, reset: bool = False) -> Tuple[float, int]:
        """(device ms, kernel launches) of the path passes since the last reset."""
        ms, n = ctypes.c_double(), ctypes.c_longlong()
        self._chk(lib.bdpt_path_timing(self._h, ctypes.byref(ms), ctypes.byref(n), int(reset)))
        return ms.value, n.value

    def kernel_timing(self, reset: bool = False) -> Tuple[float, int]:
        """(ms inside the path kernels alone, launches) since the last reset."""
        ms, n = ctypes.c_double(), ctypes.c_longlong()
        self._chk(lib.bdpt_kernel_timing(self._h, ctypes.byref(ms), ctypes.byref(n), int(reset)))
        return ms.value, n.value

    def device_timing(self) -> list:
        """Per device of the context (devices[0] first): {device, kernel_ms, path_ms, launches,
        owned_pixels} since the last timing reset (bdpt_device_timing; no reset)."""
        out = []
        for k in range(self.num_devices):
            d, km, pm = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
            n, own = ctypes.c_longlong(), ctypes.c_longlong()
            self._chk(lib.bdpt_device_timing(self._h, k, ctypes.byref(d), ctypes.byref(km), ctypes.byref(pm),
                                             ctypes.byref(n), ctypes.byref(own)))
            out.append({"device": d.value, "kernel_ms": km.value, "path_ms": pm.value,
                        "launches": n.value, "owned_pixels": own.value})
        return out

    def update_pixels(self) -> None:
        self._chk(lib.bdpt_update_pixels(self._h))

    # -- read-back
    def read_radiance(self) -> Tuple[np.ndarray, np.ndarray]:
        col = np.empty((self.height, self.width, 3), np.float32)
        cnt = np.empty((self.height, self.width), np.uint32)
        self._chk(lib.bdpt_read_radiance(self._h, _ptr(col), _ptr(cnt)))
        return col, cnt

    def write_radiance(self, colors: np.ndarray, counter: np.ndarray) -> None:
        """Upload an accumulation state (the counterpart of read_radiance); pixels follow."""
        col = np.ascontiguousarray(colors, np.float32).reshape(self.height, self.width, 3)
        cnt = np.ascontiguousarray(counter, np.uint32).reshape(self.height, self.width)
        self._chk(lib.bdpt_write_radiance(self._h, _ptr(col), _ptr(cnt)))

    def save_checkpoint(self, path: str, host_state: bytes = b"") -> None:
        buf = ctypes.create_string_buffer(host_state, len(host_state)) if host_state else None
        self._chk(lib.bdpt_save_checkpoint(self._h, os.fsencode(path), buf, len(host_state)))

    def load_checkpoint(self, path: str, host_bytes: int = 0) -> bytes:
        """Restore the render state saved with the frame -- scene, camera, MT table (by its seed),
        VLPs -- and the accumulation (bdpt_load_checkpoint); self.spheres and self.camera follow
        the restored values.  Returns the caller state saved with it (host_bytes long)."""
        buf = ctypes.create_string_buffer(host_bytes) if host_bytes else None
        self._chk(lib.bdpt_load_checkpoint(self._h, os.fsencode(path), buf, host_bytes))
        self.spheres = self.get_scene()
        cam = self.get_camera()
        if cam is not None:
            self.camera = cam
        return buf.raw if buf is not None else b""

    def read_pixels(self) -> np.ndarray:
        px = np.empty((self.height, self.width, 4), np.uint8)
        self._chk(lib.bdpt_read_pixels(self._h, _ptr(px)))
        return px

    def read_rand(self) -> np.ndarray:
        t = np.empty(RAND_N, np.float32)
        self._chk(lib.bdpt_read_rand(self._h, _ptr(t)))
        return t

    def write_rand(self, table) -> None:
        """Upload a whole random table ([RAND_N] float32; bdpt_write_rand): tests render on tables no
        seed produces."""
        t = np.ascontiguousarray(table, np.float32)
        assert t.shape == (RAND_N,)
        self._chk(lib.bdpt_write_rand(self._h, _ptr(t)))

    def read_sample_records(self) -> np.ndarray:
        """The sample records of the current table, [RAND_N - 5, 8] = {A, B, C, u2, X, Y, Z, u0} per
        position (include/bdpt.h bdpt_read_sample_records)."""
        rec = np.empty((RAND_N - 5, 8), np.float32)
        self._chk(lib.bdpt_read_sample_records(self._h, _ptr(rec)))
        return rec

    def read_lightpaths(self) -> np.ndarray:
        lp = np.empty(LIGHT_POINTS, LIGHTPATH_DTYPE)
        self._chk(lib.bdpt_read_lightpaths(self._h, _ptr(lp)))
        return lp

    def write_lightpaths(self, lp: np.ndarray) -> None:
        lp = np.ascontiguousarray(lp, LIGHTPATH_DTYPE)
        assert lp.shape == (LIGHT_POINTS,)
        self._chk(lib.bdpt_write_lightpaths(self._h, _ptr(lp)))

    def rand_seed(self) -> Optional[int]:
        """Seed of the current MT607 table (None before the first light pass)."""
        s = ctypes.c_uint()
        return int(s.value) if lib.bdpt_rand_seed(self._h, ctypes.byref(s)) == BDPT_OK else None

    def get_camera(self) -> Optional[Camera]:
        cam = Camera()
        return cam if lib.bdpt_get_camera(self._h, ctypes.byref(cam)) == BDPT_OK else None

    def get_scene(self) -> np.ndarray:
        n = lib.bdpt_get_scene(self._h, None, 0)
        if n < 0:
            raise BdptError(n, lib.bdpt_last_error(self._h).decode())
        arr = np.zeros(n, SPHERE_DTYPE)
        if n:
            lib.bdpt_get_scene(self._h, _sphere_ptr(arr), n)
        return arr

    # -- first-hit feature buffers (no reference counterpart; include/bdpt.h bdpt_render_aov)
    def render_aov(self, sid: Optional[int] = None, window: Optional[Tuple[int, int, int, int]] = None,
                   planes: Sequence[str] = AOV_PLANES) -> dict:
        """The first hit of every pixel's camera ray, in the path kernel's arithmetic: a dict of
        id [h, w] int32 (-1 = miss), t, dp [h, w] float32 and position, normal, dir [h, w, 3]
        float32.  sid=None: the unjittered pixel-centre rays (no random table needed); else the
        jitter of a pass with that sid on the current table.  window=(x0, y0, w, h): only those
        pixels (equal to that slice of the whole frame).  Changes nothing else of the context."""
        x0, y0, w, h = (0, 0, self.width, self.height) if window is None else (int(v) for v in window)
        shape = (max(h, 0), max(w, 0))
        out = {k: np.empty(shape + ((3,) if k in ("position", "normal", "dir") else ()),
                           np.int32 if k == "id" else np.float32) for k in AOV_PLANES if k in planes}
        buf = AovBuffers(**{k: a.ctypes.data for k, a in out.items()})
        self._chk(lib.bdpt_render_aov(self._h, x0, y0, w, h, int(sid is not None), int(sid or 0),
                                      ctypes.byref(buf)))
        return out

    def pick(self, x: int, y: int, sid: Optional[int] = None) -> Tuple[int, float]:
        """(sphere index or -1, hit distance) of the pixel (x, y): bdpt_pick, a 1x1 window."""
        i, t = ctypes.c_int(), ctypes.c_float()
        self._chk(lib.bdpt_pick(self._h, int(x), int(y), int(sid is not None), int(sid or 0),
                                ctypes.byref(i), ctypes.byref(t)))
        return i.value, t.value

    @property
    def last_aov_traversal(self) -> str:
        """'brute' or 'bvh': what the last render_aov / pick call traversed."""
        rc = int(lib.bdpt_last_aov_traversal(self._h))
        if rc < 0:
            raise BdptError(rc, "no feature buffers rendered yet")
        return {1: "brute", 2: "bvh"}[rc]

    def last_aov_ms(self) -> float:
        """Device time (ms) of the last render_aov / pick kernel alone, without the read-back."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_aov_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- chain buffers (no reference counterpart; include/bdpt.h bdpt_render_chain)
    def render_chain(self, sid: Optional[int] = None, branch: str = "transmit",
                     window: Optional[Tuple[int, int, int, int]] = None,
                     planes: Sequence[str] = CHAIN_PLANES) -> dict:
        """Every pixel's eye path up to its first non-specular vertex -- what the pixel shows through
        mirrors and glass -- in the path kernel's arithmetic: a dict of id (the end sphere, -1 for a
        miss or an exhausted chain), first_id (render_aov's id), kind (CHAIN_KIND_*), bounces
        [h, w] int32, t (the summed distance), dp [h, w] float32 and position, normal (of the end
        vertex), dir, throughput [h, w, 3] float32.  sid, window as for render_aov.  branch: what
        glass does -- "transmit" refracts whenever refraction exists, "pass" takes the choice the
        pass with that sid makes (needs sid).  Changes nothing else of the context."""
        x0, y0, w, h = (0, 0, self.width, self.height) if window is None else (int(v) for v in window)
        shape = (max(h, 0), max(w, 0))
        out = {k: np.empty(shape + ((3,) if k in ("position", "normal", "dir", "throughput") else ()),
                           np.int32 if k in ("id", "first_id", "kind", "bounces") else np.float32)
               for k in CHAIN_PLANES if k in planes}
        buf = ChainBuffers(**{k: a.ctypes.data for k, a in out.items()})
        self._chk(lib.bdpt_render_chain(self._h, x0, y0, w, h, int(sid is not None), int(sid or 0),
                                        CHAIN_BRANCHES.get(branch, -1) if isinstance(branch, str) else int(branch),
                                        ctypes.byref(buf)))
        return out

    def last_chain_ms(self) -> float:
        """Device time (ms) of the last render_chain kernel alone, without the read-back."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_chain_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- denoiser (no reference counterpart; include/bdpt.h bdpt_denoise)
    def denoise(self, levels: int = 4, normal_power: int = 5, sigma_color: float = 0.5,
                materials: str = "diffuse", pixels: bool = False):
        """The accumulated radiance as it stands, through an edge-avoiding wavelet filter guided by
        the unjittered first hit's sphere id and normal: `levels` a-trous levels (1..8, steps 1, 2,
        4, ...), the normals' cosine squared `normal_power` times (0..6), colour stopping
        1 / (1 + |dc|^2 4^k / sigma_color^2) (sigma_color > 0; inf: none).  materials="diffuse"
        filters only pixels that show a DIFF sphere, "all" every hit; "through" takes the guides
        from render_chain instead -- pixels whose chain through mirrors and glass ends on a diffuse
        surface, matched by what they show and through what; the others are copied through.
        Returns the [H, W, 3] float32 frame, or (frame, rgba [H, W, 4] uint8 through read_pixels'
        thresholds) with pixels=True.  Changes nothing else of the context."""
        prm = DenoiseParams(int(levels), int(normal_power), float(sigma_color), DENOISE_MATERIALS[materials])
        col = np.empty((self.height, self.width, 3), np.float32)
        px = np.empty((self.height, self.width, 4), np.uint8) if pixels else None
        self._chk(lib.bdpt_denoise(self._h, ctypes.byref(prm), _ptr(col), _ptr(px) if pixels else None))
        return (col, px) if pixels else col

    def last_denoise_ms(self) -> float:
        """Device time (ms) of the last denoise call's kernels alone, without the read-back."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_denoise_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- temporal reprojection (no reference counterpart; include/bdpt.h bdpt_reproject)
    @staticmethod
    def _reproject_params(max_history: float = 64.0, plane_tol: float = 0.01, materials: str = "diffuse"):
        return ReprojectParams(DENOISE_MATERIALS[materials], float(max_history), float(plane_tol))

    def history_capture(self, **params) -> None:
        """Take the frame as it stands (blended with the history present, if any, as reproject()
        would) as the new history under the current camera and scene.  Call it before the camera
        changes.  Parameters as for reproject()."""
        prm = self._reproject_params(**params)
        self._chk(lib.bdpt_history_capture(self._h, ctypes.byref(prm)))

    def history_clear(self) -> None:
        self._chk(lib.bdpt_history_clear(self._h))

    def history_follow(self, on: bool = True) -> None:
        """Opt in to (or out of) a history that follows moved spheres: one taken under spheres that
        differ from the current ones only by translations of non-emitting spheres stays present,
        and a pixel on a moved sphere fetches its history where that sphere was (include/bdpt.h
        bdpt_history_follow).  Off by default; the switch survives set_scene, set_camera and
        reset_accum."""
        self._chk(lib.bdpt_history_follow(self._h, int(bool(on))))

    def history_motion(self) -> Tuple[int, Optional[np.ndarray]]:
        """(state, delta): the stored history against the current spheres, whether history_follow is
        on or off -- 0 none stored, 1 the spheres are the same bytes, 2 followable, 3 not usable --
        and in states 1 and 2 the spheres' offsets from the history's, [n, 3] float32 (else None)."""
        n = lib.bdpt_get_scene(self._h, None, 0)
        state = ctypes.c_int(-1)
        delta = np.zeros((max(n, 0), 3), np.float32)
        self._chk(lib.bdpt_history_motion(self._h, ctypes.byref(state), _ptr(delta), max(n, 0)))
        return state.value, (delta if state.value in (1, 2) else None)

    def history_info(self) -> Tuple[bool, Optional[Camera]]:
        """(present, camera): whether a history is stored and the scene is still the one it was
        taken under (with history_follow on: or one it can follow), and the camera of the stored
        history (None if none was ever stored)."""
        present, cam = ctypes.c_int(-1), Camera()
        cam.orig.x = float("nan")
        self._chk(lib.bdpt_history_info(self._h, ctypes.byref(present), ctypes.byref(cam)))
        return bool(present.value), (None if cam.orig.x != cam.orig.x else cam)

    def history_read(self) -> Tuple[np.ndarray, np.ndarray]:
        """The stored history's colours [H, W, 3] float32 and weights [H, W] float32."""
        col = np.empty((self.height, self.width, 3), np.float32)
        w = np.empty((self.height, self.width), np.float32)
        self._chk(lib.bdpt_history_read(self._h, _ptr(col), _ptr(w)))
        return col, w

    def history_write(self, camera: Camera, colors, weight) -> None:
        """Upload a history: colours and per-pixel weights taken under `camera` and the current
        scene (its guides are rendered here)."""
        col = np.ascontiguousarray(colors, np.float32).reshape(self.height, self.width, 3)
        w = np.ascontiguousarray(weight, np.float32).reshape(self.height, self.width)
        self._chk(lib.bdpt_history_write(self._h, ctypes.byref(camera), _ptr(col), _ptr(w)))

    def reproject(self, max_history: float = 64.0, plane_tol: float = 0.01, materials: str = "diffuse",
                  weight: bool = False, pixels: bool = False):
        """The preview after a camera move: the accumulated radiance as it stands, blended by sample
        count with the history fetched where the old view showed the same surface (the pixel's first
        hit projected into the history's camera, four bilinear taps validated by sphere id and a
        plane test of plane_tol x hit distance, each tap's weight capped at max_history).
        materials="diffuse" takes history only on DIFF spheres.  Returns the [H, W, 3] float32 frame,
        followed by the [H, W] float32 blended sample count with weight=True and by the rgba
        [H, W, 4] uint8 (read_pixels' thresholds) with pixels=True.  Changes nothing else of the
        context; without a history it returns read_radiance()."""
        prm = self._reproject_params(max_history, plane_tol, materials)
        col = np.empty((self.height, self.width, 3), np.float32)
        w = np.empty((self.height, self.width), np.float32) if weight else None
        px = np.empty((self.height, self.width, 4), np.uint8) if pixels else None
        self._chk(lib.bdpt_reproject(self._h, ctypes.byref(prm), _ptr(col), _ptr(w) if weight else None,
                                     _ptr(px) if pixels else None))
        out = (col,) + ((w,) if weight else ()) + ((px,) if pixels else ())
        return out if len(out) > 1 else col

    def last_reproject_ms(self) -> float:
        """Device time (ms) of the last reproject / history_capture call's kernels alone."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_reproject_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- the reprojected preview, denoised (no reference counterpart; include/bdpt.h bdpt_preview_denoise)
    def preview_denoise(self, levels: int = 4, normal_power: int = 5, sigma_color: float = 0.5,
                        count_ref: float = 8.0, max_history: float = 64.0, plane_tol: float = 0.01,
                        materials: str = "diffuse", weight: bool = False, pixels: bool = False):
        """reproject() and denoise() in one call that knows each pixel's sample count: the
        reprojected frame (max_history, plane_tol, materials as for reproject()) through `levels`
        a-trous levels (0..8; 0 is reproject() itself) in which a tap is weighted by its count and
        the colour stopping is scaled by a_p a_q / (a_p + a_q) * 2 / count_ref -- two pixels of
        count_ref passes each are told apart as denoise() would, pixels with more history are
        blurred less readily, one-pass pixels take their neighbours' colour.  materials selects the
        pixels for both stages.  Returns the [H, W, 3] float32 frame, followed by the [H, W]
        float32 carried sample count with weight=True and by the rgba [H, W, 4] uint8 with
        pixels=True.  Changes nothing else of the context, the history included."""
        prm = PreviewParams(self._reproject_params(max_history, plane_tol, materials), int(levels),
                            int(normal_power), float(sigma_color), float(count_ref))
        col = np.empty((self.height, self.width, 3), np.float32)
        w = np.empty((self.height, self.width), np.float32) if weight else None
        px = np.empty((self.height, self.width, 4), np.uint8) if pixels else None
        self._chk(lib.bdpt_preview_denoise(self._h, ctypes.byref(prm), _ptr(col), _ptr(w) if weight else None,
                                           _ptr(px) if pixels else None))
        out = (col,) + ((w,) if weight else ()) + ((px,) if pixels else ())
        return out if len(out) > 1 else col

    def last_preview_ms(self) -> float:
        """Device time (ms) of the last preview_denoise call's kernels alone."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_preview_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- per-tile noise estimate (no reference counterpart; include/bdpt.h bdpt_noise_estimate)
    def noise_mark(self) -> None:
        """Take the frame as it stands (colours and per-pixel counts) as the mark the next
        noise_estimate() measures against."""
        self._chk(lib.bdpt_noise_mark(self._h))

    def noise_clear(self) -> None:
        self._chk(lib.bdpt_noise_clear(self._h))

    def noise_tiles(self) -> Tuple[int, int]:
        """(tiles_x, tiles_y) of the 32 x 8 tile grid."""
        tx, ty = ctypes.c_int(), ctypes.c_int()
        self._chk(lib.bdpt_noise_tiles(self._h, ctypes.byref(tx), ctypes.byref(ty)))
        return tx.value, ty.value

    def noise_read_mark(self) -> Tuple[np.ndarray, np.ndarray]:
        """The mark's colours [H, W, 3] float32 and counts [H, W] uint32 (0: no mark)."""
        col = np.empty((self.height, self.width, 3), np.float32)
        cnt = np.empty((self.height, self.width), np.uint32)
        self._chk(lib.bdpt_noise_read_mark(self._h, _ptr(col), _ptr(cnt)))
        return col, cnt

    def noise_write_mark(self, colors, counter) -> None:
        col = np.ascontiguousarray(colors, np.float32).reshape(self.height, self.width, 3)
        cnt = np.ascontiguousarray(counter, np.uint32).reshape(self.height, self.width)
        self._chk(lib.bdpt_noise_write_mark(self._h, _ptr(col), _ptr(cnt)))

    def noise_estimate(self, dark: float = 0.01, threshold: float = 0.05, remark: bool = False,
                       pixels: bool = False) -> dict:
        """How noisy the frame is, from how far the running mean has moved since the mark: per
        pixel (|B - A| summed over the channels) * sqrt(mn / (cnt - mn)) / sqrt(max(B's channel sum,
        dark)), valid where the samples since the mark are at least half the marked ones; averaged
        over 32 x 8 tiles.  remark=True lets every pixel whose count has doubled since its mark (or
        that has none) take the present frame as its mark afterwards.  Returns the summary
        (valid_pixels, pending_pixels, tiles_x, tiles_y, valid_tiles, tiles_over, mean, max_tile)
        with tile_error float32 and tile_valid uint32 as [tiles_y, tiles_x] arrays, and with
        pixels=True error as [H, W] float32 (-1 where not valid).  Changes nothing of the context
        but the mark."""
        prm = NoiseParams(float(dark), float(threshold), int(bool(remark)))
        tx, ty = self.noise_tiles()
        err = np.empty((self.height, self.width), np.float32) if pixels else None
        te = np.empty((ty, tx), np.float32)
        tv = np.empty((ty, tx), np.uint32)
        sm = NoiseSummary()
        self._chk(lib.bdpt_noise_estimate(self._h, ctypes.byref(prm), _ptr(err) if pixels else None, _ptr(te),
                                          _ptr(tv), ctypes.byref(sm)))
        out = {name: getattr(sm, name) for name, _ in NoiseSummary._fields_}
        out["tile_error"], out["tile_valid"] = te, tv
        if pixels:
            out["error"] = err
        return out

    def noise_tile_pending(self) -> np.ndarray:
        """The last noise_estimate's pending pixels per tile, [tiles_y, tiles_x] uint32: pixels with
        0 < count < 30000 that are not valid yet (their sum is the summary's pending_pixels)."""
        tx, ty = self.noise_tiles()
        tp = np.empty((ty, tx), np.uint32)
        self._chk(lib.bdpt_noise_tile_pending(self._h, _ptr(tp)))
        return tp

    def last_noise_ms(self) -> float:
        """Device time (ms) of the last noise_estimate call's kernel alone."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_noise_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # -- noise-guided denoiser (no reference counterpart; include/bdpt.h bdpt_denoise_noise)
    def denoise_noise(self, levels: int = 4, normal_power: int = 5, sigma_color: float = 0.5,
                      noise_sigma: float = 1.0, materials: str = "diffuse", pixels: bool = False,
                      variance: bool = False):
        """denoise() with a colour stop that follows the measured noise: where the mark (noise_mark,
        or noise_estimate(remark=True)) gives a pixel a variance estimate -- |B - A|^2 mn / (cnt - mn),
        valid as for noise_estimate, averaged over the 5 x 5 neighbours on the same sphere -- two
        pixels' colours stop each other by t / (t + |dc|^2) with t = noise_sigma^2 (v_p + v_q) + 1e-12,
        and the variance is carried through the levels; where it does not, by denoise()'s
        sigma_color.  A converged frame is therefore left alone and a noisy one filtered hard.
        Without a mark, or with one that is valid nowhere, the result is denoise()'s, bit for bit.
        Returns the [H, W, 3] float32 frame; with pixels=True and / or variance=True a tuple
        (frame[, rgba [H, W, 4] uint8][, variance [H, W] float32, -1 where there is none]).  Reads
        the accumulation, the counters and the mark; changes nothing of the context."""
        prm = DenoiseNoiseParams(int(levels), int(normal_power), float(sigma_color), DENOISE_MATERIALS[materials],
                                 float(noise_sigma))
        col = np.empty((self.height, self.width, 3), np.float32)
        px = np.empty((self.height, self.width, 4), np.uint8) if pixels else None
        var = np.empty((self.height, self.width), np.float32) if variance else None
        self._chk(lib.bdpt_denoise_noise(self._h, ctypes.byref(prm), _ptr(col), _ptr(px) if pixels else None,
                                         _ptr(var) if variance else None))
        if not pixels and not variance:
            return col
        return (col,) + ((px,) if pixels else ()) + ((var,) if variance else ())

    def last_denoise_noise_ms(self) -> float:
        """Device time (ms) of the last denoise_noise call's kernels alone, without the read-back."""
        ms = ctypes.c_float()
        self._chk(lib.bdpt_last_denoise_noise_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def device_buffers(self) -> Tuple[int, int, int]:
        c, n, p = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(lib.bdpt_device_buffers(self._h, ctypes.byref(c), ctypes.byref(n), ctypes.byref(p)))
        return c.value, n.value, p.value

    # -- optional display: HIP-GL interop of the caller's pixel-unpack buffer
    def gl_register_pbo(self, pbo: int) -> None:
        """cudaGLRegisterBufferObject (smallpt_cpu.c:122): needs a current OpenGL context."""
        self._chk(lib.bdpt_gl_register_pbo(self._h, int(pbo)))

    def gl_publish(self) -> None:
        """IdleFunc's map / render / unmap (display_func.c:199-215): the frame's pixels into the PBO."""
        self._chk(lib.bdpt_gl_publish(self._h))

    def gl_unregister(self) -> None:
        self._chk(lib.bdpt_gl_unregister(self._h))


# ---- the reference's operator interface (smallpt_cpu.c / display_func.c) --------------------

class SmallPT:
    """Mirror of smallpt_cpu.c's module state and functions, headless.

    SmallPT(w, h, scene) behaves like `smallptCPU <w> <h> <scene>`: sizes get +1
    (smallpt_cpu.c:409-410), UpdateCamera, AllocateBuffers.  IdleFunc() is one frame of the GLUT
    idle loop (display_func.c:192-217); KeyFunc/SpecialFunc replay the keyboard handlers.
    """

    def __init__(self, width: Optional[int] = None, height: Optional[int] = None,
                 scene: Optional[str] = None, device: int = 0, dat_path: str = DEFAULT_DAT,
                 reuse_history: bool = False, follow_spheres: bool = False):
        # reuse_history: camera keys capture the frame before ReInit discards it, so that preview()
        # can reproject it into the new view (Renderer.reproject); the render path is unchanged
        # follow_spheres (with reuse_history): sphere and selection keys capture the frame too instead
        # of clearing the history, which then follows the moved sphere (Renderer.history_follow)
        self.reuse_history = bool(reuse_history)
        self.follow_spheres = bool(follow_spheres)
        if self.follow_spheres and not self.reuse_history:
            raise ValueError("follow_spheres=True needs reuse_history=True")
        if scene is not None:
            self.camera, self.spheres = read_scene(scene)
            self.width, self.height = int(width), int(height)
        else:
            self.camera, self.spheres = default_scene()
            self.width, self.height = 640, 480
        self.height += 1
        self.width += 1
        update_camera(self.camera, self.width, self.height)
        self.device, self.dat_path = device, dat_path
        self.current_sample = 0
        self.reinit_counter = 0
        self.current_sphere = 0
        self.total_time = 0.0
        self.sched = PassScheduler()
        self.renderer: Optional[Renderer] = None
        self.AllocateBuffers()

    @property
    def flag(self) -> int:
        return self.sched.flag

    def AllocateBuffers(self) -> None:                       # smallpt_cpu.c:153
        if self.renderer is None:
            self.renderer = Renderer(self.spheres, self.width, self.height, self.camera,
                                     self.dat_path, self.device)
            if self.follow_spheres:
                self.renderer.history_follow(True)
        else:                                                 # buffers persist (Appendix A.6)
            self.renderer.reset_accum()
            self.renderer.set_scene(self.spheres)

    def FreeBuffers(self) -> None:                           # smallpt_cpu.c:98
        if self.renderer is not None:
            self.renderer.close()
            self.renderer = None

    def UpdateRendering2(self) -> None:                      # smallpt_cpu.c:300-362
        self.renderer.light_pass(self.current_sample)
        self.sched.light()

    def UpdateRendering(self, npass: int = 1, tiles=None) -> float:   # smallpt_cpu.c:265-297 (x npass)
        """tiles (no reference counterpart): render only these 32 x 8 tiles (Renderer.path_passes);
        the pass schedule and current_sample advance by npass either way, and the returned samples
        per second count the masked tiles' pixels inside the frame."""
        import time
        sid, vlp = self.sched.next(npass)
        t0 = time.perf_counter()
        self.renderer.path_passes(sid, vlp, tiles=tiles)
        dt = time.perf_counter() - t0
        self.current_sample += npass
        # static float total_time; total_time += (float)elapsed (smallpt_cpu.c:35,283)
        self.total_time = float(np.float32(np.float32(self.total_time) + np.float32(dt)))
        npix = self.width * self.height if tiles is None else self.tile_pixels(tiles)
        return npix * npass / dt if dt > 0 else float("inf")

    def tile_pixels(self, tiles) -> int:
        """The pixels inside the frame of the 32 x 8 tiles with a non-zero entry in `tiles`."""
        mask = self.renderer._tile_mask(tiles).astype(bool)
        w = np.minimum(32, self.width - 32 * np.arange(mask.shape[1]))
        h = np.minimum(8, self.height - 8 * np.arange(mask.shape[0]))
        return int((np.outer(h, w) * mask).sum())

    def IdleFunc(self, npass: int = 1, tiles=None) -> None:  # display_func.c:192-217
        if self.flag == 1:
            self.UpdateRendering2()
        if self.flag > 1:
            self.UpdateRendering(npass, tiles)

    def RenderUntil(self, threshold: float = 0.05, max_passes: int = 4096, batch: int = 8,
                    dark: float = 0.01, pixels: bool = False, adaptive: bool = False, min_passes: int = 0,
                    denoise: bool = False, **denoise_params) -> dict:
        """Render until the frame is good enough instead of a fixed number of passes (no reference
        counterpart): IdleFunc(batch), then Renderer.noise_estimate(remark=True), repeated.  Stops
        as converged when some pixel is valid, none is pending and no tile's error is over
        `threshold`; as not converged once current_sample >= max_passes.  Returns the last
        estimate's dict (pixels=True: with its per-pixel `error`) with `passes` (current_sample)
        and `converged`.  The frame is exactly what
        the same IdleFunc(batch) calls render.  ReInit and ReInitScene clear the mark through the
        calls they make.

        adaptive=True stops each 32 x 8 tile on its own instead of rendering every pixel until the
        worst tile is good enough: IdleFunc(batch, tiles=the tiles not retired), the estimate, and
        then every tile not yet retired retires if none of its pixels is pending, its error is at
        most `threshold` (or it has no valid pixel: nothing in it is being sampled) and
        current_sample >= min_passes.  A retired tile stays retired: it is not rendered again, so
        its pixels hold what the unmasked frame held after retired_at passes.  Stops as converged
        when every tile is retired.  The dict then also carries retired_at (int32, the
        current_sample a tile retired at, 0: not retired), retired_error (float32, its error then)
        and pixel_passes (the sum over batches of batch x pixels rendered).  The frame is noisier
        than the unmasked one at the same stop: that one oversamples the easy tiles (DESIGN.md 4h;
        min_passes guards tiles that look settled after very few passes).

        denoise=True also returns the frame through the noise-guided filter as `denoised`
        (Renderer.denoise_noise(**denoise_params); its variance plane as `denoised_variance`).  A pixel that has just re-marked has no fresh
        samples and so no variance estimate, so on this path every check estimates with remark=False
        first; when the loop is about to stop it filters and returns, with the mark the filter
        used still in place, otherwise it repeats the estimate with remark=True.  Passes, estimate
        and frame are those of the call without it.  Not with adaptive=True."""
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if denoise and adaptive:
            raise ValueError("denoise=True is not available with adaptive=True")
        if denoise_params and not denoise:
            raise TypeError(f"unexpected arguments without denoise=True: {sorted(denoise_params)}")
        if adaptive:
            return self._render_until_adaptive(threshold, max_passes, batch, dark, pixels, min_passes)
        while True:
            self.IdleFunc(batch)
            est = self.renderer.noise_estimate(dark=dark, threshold=threshold, remark=not denoise, pixels=pixels)
            converged = est["valid_pixels"] > 0 and est["pending_pixels"] == 0 and est["tiles_over"] == 0
            if converged or self.current_sample >= max_passes:
                if denoise:
                    est["denoised"], est["denoised_variance"] = self.renderer.denoise_noise(variance=True, **denoise_params)
                break
            if denoise:
                self.renderer.noise_estimate(dark=dark, threshold=threshold, remark=True)
        est["passes"] = self.current_sample
        est["converged"] = bool(converged)
        return est

    def _render_until_adaptive(self, threshold, max_passes, batch, dark, pixels, min_passes) -> dict:
        tx, ty = self.renderer.noise_tiles()
        retired_at = np.zeros((ty, tx), np.int32)
        retired_error = np.zeros((ty, tx), np.float32)
        pixel_passes = 0
        while True:
            live = retired_at == 0
            first = self.current_sample
            self.IdleFunc(batch, tiles=live)
            pixel_passes += (self.current_sample - first) * self.tile_pixels(live)
            est = self.renderer.noise_estimate(dark=dark, threshold=threshold, remark=True, pixels=pixels)
            pending = self.renderer.noise_tile_pending()
            settled = (est["tile_valid"] == 0) | (est["tile_error"] <= np.float32(threshold))
            retire = live & (pending == 0) & settled & (self.current_sample >= min_passes)
            retired_at[retire] = self.current_sample
            retired_error[retire] = est["tile_error"][retire]
            converged = bool((retired_at != 0).all())
            if converged or self.current_sample >= max_passes:
                break
        est["passes"] = self.current_sample
        est["converged"] = converged
        est["retired_at"], est["retired_error"], est["pixel_passes"] = retired_at, retired_error, int(pixel_passes)
        return est

    def ReInit(self, realloc: bool = True) -> None:          # smallpt_cpu.c:373-387
        if realloc:
            self.AllocateBuffers()
        self.reinit_counter += 1
        update_camera(self.camera, self.width, self.height)
        self.renderer.set_camera(self.camera)
        self.current_sample = 0
        if self.reinit_counter % 2 == 0:
            self.UpdateRendering2()
        self.UpdateRendering(1)

    def ReInitScene(self) -> None:                           # smallpt_cpu.c:365-371
        if self.follow_spheres:                               # the context still holds the old spheres
            self.renderer.history_capture()
        elif self.reuse_history:                              # a moved sphere changes the lighting everywhere
            self.renderer.history_clear()
        self.current_sample = 0
        self.sched.state.flag = 1
        self.AllocateBuffers()
        self.UpdateRendering2()

    def KeyFunc(self, key: str) -> None:                     # display_func.c:278-382
        if key in "+-":
            n = len(self.spheres)
            self.current_sphere = (self.current_sphere + (1 if key == "+" else n - 1)) % n
            self.ReInitScene()
        elif key in "468293":
            if sphere_key(self.spheres, self.current_sphere, key):
                self.ReInitScene()
        elif camera_key(self.camera, key):
            if self.reuse_history:                            # the context still holds the old camera
                self.renderer.history_capture()
            self.ReInit(True)

    def PickSphere(self, x: int, y: int) -> int:
        """Select the sphere the pixel (x, y) shows (no reference counterpart: its only selection is
        the '+'/'-' cycle, display_func.c:336-343).  On a hit current_sphere becomes that sphere and
        the scene is re-initialised as the '+'/'-' handlers do; on a miss nothing changes.  Returns
        the sphere index or -1."""
        sphere, _ = self.renderer.pick(x, y)
        if sphere >= 0:
            self.current_sphere = sphere
            self.ReInitScene()
        return sphere

    def SpecialFunc(self, key: str) -> None:                 # display_func.c:384-437
        if camera_key(self.camera, key):
            if self.reuse_history:
                self.renderer.history_capture()
            self.ReInit(True)

    def colors(self) -> Tuple[np.ndarray, np.ndarray]:
        return self.renderer.read_radiance()

    def pixels(self) -> np.ndarray:
        return self.renderer.read_pixels()

    _STATE = struct.Struct("<35i3if")          # bdpt_pass_state (31 + f, r, flag, vlp) + 3 ints + float

    def SaveCheckpoint(self, path: str) -> None:
        """Accumulation + pass schedule + host counters (no reference counterpart)."""
        st = self.sched.state
        words = list(st.rng.state) + [st.rng.f, st.rng.r, st.flag, st.vlp_index]
        blob = self._STATE.pack(*words, self.current_sample, self.reinit_counter, self.current_sphere,
                                self.total_time)
        self.renderer.save_checkpoint(path, blob)

    def LoadCheckpoint(self, path: str) -> None:
        """Restore what SaveCheckpoint wrote; rendering continues bit for bit.  The checkpoint
        carries the render state too (camera, spheres, MT table seed, VLPs -- keys may have
        edited them before the save): the context restores it, and the mirror takes over the
        camera and spheres, so later keys continue from the saved state."""
        v = self._STATE.unpack(self.renderer.load_checkpoint(path, self._STATE.size))
        cam = self.renderer.get_camera()
        if cam is not None:
            self.camera = cam
        self.spheres = self.renderer.get_scene()
        self.renderer.spheres = self.spheres
        st = self.sched.state
        for k in range(31):
            st.rng.state[k] = v[k]
        st.rng.f, st.rng.r, st.flag, st.vlp_index = v[31:35]
        self.current_sample, self.reinit_counter, self.current_sphere = v[35:38]
        self.total_time = v[38]

    def SavePPM(self, path: Optional[str] = None, binary: bool = False) -> str:   # smallpt_cpu.c:239-262
        if path is None:
            path = ppm_name(self.total_time, self.current_sample)
        save_ppm(path, self.pixels(), binary)
        return path

    def SaveDenoisedPPM(self, path: Optional[str] = None, binary: bool = False, noise: bool = False, **params) -> str:
        """SavePPM of the denoised frame (Renderer.denoise(**params)); without a path, SavePPM's
        file name with `_denoised` before `.ppm`.  noise=True: of the noise-guided filter's frame
        (Renderer.denoise_noise(**params)), named `_denoised_noise`."""
        if path is None:
            suffix = "_denoised_noise.ppm" if noise else "_denoised.ppm"
            path = ppm_name(self.total_time, self.current_sample)[:-len(".ppm")] + suffix
        call = self.renderer.denoise_noise if noise else self.renderer.denoise
        _, px = call(pixels=True, **params)
        save_ppm(path, px, binary)
        return path

    def preview(self, denoise: bool = False, **params):
        """The frame with the last view's history reprojected into it (Renderer.reproject(**params));
        with reuse_history=False there is no history and this is the raw frame.  denoise=True: the
        same through the count-weighted filter (Renderer.preview_denoise(**params))."""
        if denoise:
            return self.renderer.preview_denoise(**params)
        return self.renderer.reproject(**params)

    def SavePreviewPPM(self, path: Optional[str] = None, binary: bool = False, denoise: bool = False,
                       **params) -> str:
        """SavePPM of the preview's pixels; without a path, SavePPM's file name with `_preview`
        (denoise=True: `_preview_denoised`) before `.ppm`."""
        if path is None:
            suffix = "_preview_denoised.ppm" if denoise else "_preview.ppm"
            path = ppm_name(self.total_time, self.current_sample)[:-len(".ppm")] + suffix
        call = self.renderer.preview_denoise if denoise else self.renderer.reproject
        px = call(pixels=True, **params)[-1]
        save_ppm(path, px, binary)
        return path
