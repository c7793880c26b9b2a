"""REFERENCE BUILD -- test infrastructure only (tests/test_ref_parity.py, tests/golden/make_ref_golden.py).

ctypes wrapper of oracle/_ref/libref.so: the reference's own src/device.cu and
src/MersenneTwister_kernel.cu compiled in place as host C++ (Makefile, oracle/ref_shim.h,
oracle/ref_driver.cpp), with the array conventions of oracle/__init__.py.  The library exists only
where the reference tree does (BDPT_REFERENCE, default /root/reference); it is never committed, and
neither the product, bench.py nor smoke() loads it.

`ref` is the correctly rounded build (cos/sin/pow as (float)f((double)x), the project's
floating-point contract); `ref_libm()` is the second build, whose cos/sin/pow are the platform's
float overloads (measured in DESIGN.md "Oracle", not a checker).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_HERE)
REFERENCE = os.environ.get("BDPT_REFERENCE", "/root/reference")
LIB_PATH = os.path.join(_HERE, "_ref", "libref.so")
LIBM_LIB_PATH = os.path.join(_HERE, "_ref", "libref_libm.so")
HOST_LIB_PATH = os.path.join(_HERE, "_ref", "libref_host.so")
DEFAULT_DAT = os.path.join(_REPO, "assets", "data", "MersenneTwister.dat")
RAND_N = 4096 * 1876
LIGHT_POINTS = 4096

SPHERE_DTYPE = np.dtype([("rad", "<f4"), ("p", "<f4", 3), ("e", "<f4", 3), ("c", "<f4", 3),
                         ("refl", "<i4")])
LIGHTPATH_DTYPE = np.dtype([("hp", "<f4", 3), ("rad", "<f4", 3), ("nl", "<f4", 3)])
CAMERA_DTYPE = np.dtype([("orig", "<f4", 3), ("target", "<f4", 3), ("dir", "<f4", 3),
                         ("x", "<f4", 3), ("y", "<f4", 3)])


def have_reference() -> bool:
    return os.path.isfile(os.path.join(REFERENCE, "src", "device.cu"))


def available() -> bool:
    """True when libref.so is there or can be built from the reference tree."""
    return os.path.exists(LIB_PATH) or have_reference()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _camera_array(cam) -> np.ndarray:
    if isinstance(cam, np.ndarray):
        return np.ascontiguousarray(cam.astype(CAMERA_DTYPE, copy=False).reshape(1))
    a = np.zeros(1, CAMERA_DTYPE)
    ctypes.memmove(a.ctypes.data, ctypes.addressof(cam), CAMERA_DTYPE.itemsize)
    return a


def _open(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        if not have_reference():
            raise FileNotFoundError(f"{path} is missing and there is no reference tree at {REFERENCE}")
        subprocess.check_call(["make", "-s", os.path.relpath(path, _REPO), "BDPT_REFERENCE=" + REFERENCE],
                              cwd=_REPO)
    return ctypes.CDLL(path)


class RefLib:
    def __init__(self, path: str):
        self.path = path
        self.lib = lib = _open(path)
        P = ctypes.c_void_p
        lib.ref_mt607.argtypes = [ctypes.c_char_p, ctypes.c_uint, P]
        lib.ref_mt607.restype = ctypes.c_int
        lib.ref_light_pass.argtypes = [P, ctypes.c_uint, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, P]
        lib.ref_light_pass.restype = None
        lib.ref_path_passes.argtypes = [P, ctypes.c_uint, P, P, ctypes.c_int, ctypes.c_int, P, P, P,
                                        ctypes.c_int, P, P, P]
        lib.ref_path_passes.restype = None
        assert lib.ref_rand_n() == RAND_N and lib.ref_light_points() == LIGHT_POINTS
        self.platform_libm = bool(lib.ref_platform_libm())

    def mt607(self, seed: int, dat_path: str = DEFAULT_DAT) -> np.ndarray:
        """loadMTGPU + seedMTGPU(seed) + RandomGPU<<<32,128>>> -> the RAND_N table."""
        out = np.empty(RAND_N, np.float32)
        if self.lib.ref_mt607(os.fsencode(dat_path), seed, _p(out)) != 0:
            raise OSError(f"cannot read {dat_path}")
        return out

    def light_pass(self, spheres, rnd, current_sample: int = 0, lp=None, cam=None,
                   width: int = 33, height: int = 25) -> np.ndarray:
        """UpdateRendering2's kernels for every emitter; rnd is the table of seed current_sample*5.
        The camera and the frame size reach the kernel but no value it stores depends on them."""
        sp = np.ascontiguousarray(spheres.astype(SPHERE_DTYPE, copy=False))
        lp = np.zeros(LIGHT_POINTS, LIGHTPATH_DTYPE) if lp is None else lp.copy()
        cam = None if cam is None else _camera_array(cam)
        self.lib.ref_light_pass(_p(sp), len(sp), _p(rnd), current_sample,
                                None if cam is None else _p(cam), width, height, _p(lp))
        return lp

    def path_passes(self, spheres, rnd, cam, width, height, lp, sid, vlp, colors=None, counter=None,
                    pixels=None):
        """len(sid) x RadiancePathTracingKernel over the whole frame -> (colors, counter, pixels)."""
        sp = np.ascontiguousarray(spheres.astype(SPHERE_DTYPE, copy=False))
        cam = _camera_array(cam)
        sid = np.ascontiguousarray(sid, np.uint32)
        vlp = np.ascontiguousarray(vlp, np.int32)
        assert sid.shape == vlp.shape and ((0 <= vlp) & (vlp < LIGHT_POINTS)).all()
        lp = np.ascontiguousarray(lp, LIGHTPATH_DTYPE)
        colors = np.zeros((height, width, 3), np.float32) if colors is None else \
            np.array(colors, np.float32).reshape(height, width, 3)
        counter = np.zeros((height, width), np.uint32) if counter is None else \
            np.array(counter, np.uint32).reshape(height, width)
        pixels = np.zeros((height, width, 4), np.uint8) if pixels is None else \
            np.array(pixels, np.uint8).reshape(height, width, 4)
        self.lib.ref_path_passes(_p(sp), len(sp), _p(rnd), _p(cam), width, height, _p(lp), _p(sid),
                                 _p(vlp), len(sid), _p(colors), _p(counter), _p(pixels))
        return colors, counter, pixels


GLUT_SPECIAL = {"left": 100, "up": 101, "right": 102, "down": 103, "page_up": 104, "page_down": 105}


class RefHost:
    """The reference's display_func.c (libref_host.so): one global scene and camera, as there."""

    def __init__(self, path: str = HOST_LIB_PATH):
        self.lib = lib = _open(path)
        P = ctypes.c_void_p
        lib.refhost_read_scene.argtypes = [ctypes.c_char_p]
        lib.refhost_read_scene.restype = ctypes.c_uint
        for f in (lib.refhost_get_camera, lib.refhost_set_camera, lib.refhost_get_spheres):
            f.argtypes = [P]
            f.restype = None
        lib.refhost_update_camera.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.refhost_update_camera.restype = None
        lib.refhost_key.argtypes = [ctypes.c_int]
        lib.refhost_special.argtypes = [ctypes.c_int]
        lib.refhost_current_sphere.restype = ctypes.c_uint
        self.count = 0

    def read_scene(self, path: str):
        """ReadScene -> (camera with orig/target set, spheres)."""
        self.count = int(self.lib.refhost_read_scene(os.fsencode(path)))
        return self.camera(), self.spheres()

    def camera(self) -> np.ndarray:
        c = np.zeros(1, CAMERA_DTYPE)
        self.lib.refhost_get_camera(_p(c))
        return c

    def set_camera(self, cam) -> None:
        self.lib.refhost_set_camera(_p(_camera_array(cam)))

    def spheres(self) -> np.ndarray:
        sp = np.zeros(self.count, SPHERE_DTYPE)
        if self.count:
            self.lib.refhost_get_spheres(_p(sp))
        return sp

    def update_camera(self, width: int, height: int) -> np.ndarray:
        self.lib.refhost_update_camera(width, height)
        return self.camera()

    def key(self, key: str):
        """KeyFunc, or SpecialFunc for a GLUT_SPECIAL name -> (ReInit calls, ReInitScene calls)."""
        rc = self.lib.refhost_special(GLUT_SPECIAL[key]) if key in GLUT_SPECIAL else \
            self.lib.refhost_key(ord(key))
        return rc & 0xFF, rc >> 8

    @property
    def current_sphere(self) -> int:
        return int(self.lib.refhost_current_sphere())


_libs: dict = {}


def ref() -> RefLib:
    if "ref" not in _libs:
        _libs["ref"] = RefLib(LIB_PATH)
        assert not _libs["ref"].platform_libm
    return _libs["ref"]


def ref_libm() -> RefLib:
    if "libm" not in _libs:
        _libs["libm"] = RefLib(LIBM_LIB_PATH)
        assert _libs["libm"].platform_libm
    return _libs["libm"]


def ref_host() -> RefHost:
    if "host" not in _libs:
        _libs["host"] = RefHost()
    return _libs["host"]
