"""Device-side host wrapper over the C ABI (include/rt_api.h).

PyTorch is plumbing only: it owns HBM buffers and streams; every pixel is computed by the HIP kernels in
lib/librt_amd.so.  There is no fallback path — a missing library or device raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import abi, scenes


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("device buffers must be contiguous HIP tensors")
    return ctypes.c_void_p(t.data_ptr())


class Tracer:
    """One rt_ctx on one device (rt_ctx_create) holding the uploaded scene (rt_set_scene)."""

    def __init__(self, device: int = 0):
        self.device = device
        self._ctx = ctypes.c_void_p()
        abi.check(abi.lib().rt_ctx_create(device, ctypes.byref(self._ctx)), "rt_ctx_create")
        self._scene = None
        self._windows = None                   # set_windows: (width, height, layout, elements) of the list in force

    def close(self):
        if self._ctx:
            abi.lib().rt_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------ scene
    def set_scene(self, scene: "scenes.Scene | abi.rt_scene"):
        s = scene.to_abi() if isinstance(scene, scenes.Scene) else scene
        abi.check(abi.lib().rt_set_scene(self._ctx, ctypes.byref(s)), "rt_set_scene")
        self._scene = scene

    # ----------------------------------------------------------------------------------------- render
    def alloc(self, width: int, height: int, rows: Optional[abi.rt_rows] = None, rgba32f=True, rgba8=False,
              rgb64f=False, raycount=False):
        nl = scenes.local_rows(height, rows)
        dev = torch.device("cuda", self.device)
        return {
            "rgba32f": torch.empty((nl, width, 4), dtype=torch.float32, device=dev) if rgba32f else None,
            "rgba8": torch.empty((nl, width, 4), dtype=torch.uint8, device=dev) if rgba8 else None,
            "rgb64f": torch.empty((nl, width, 3), dtype=torch.float64, device=dev) if rgb64f else None,
            "raycount": torch.empty((nl, width), dtype=torch.int32, device=dev) if raycount else None,
        }

    def render_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, bufs: dict,
                    rows: Optional[abi.rt_rows] = None, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_dev: asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_render_dev(self._ctx, ctypes.byref(cam), width, height, depth,
                                          ctypes.byref(rows) if rows is not None else None,
                                          _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")),
                                          _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")),
                                          ctypes.c_void_p(st.cuda_stream)), "rt_render_dev")
        return bufs

    def render(self, cam, width, height, depth, rows=None, rgba32f=True, rgba8=False, rgb64f=False,
               raycount=False, stream=None):
        bufs = self.alloc(width, height, rows, rgba32f, rgba8, rgb64f, raycount)
        return self.render_into(cam, width, height, depth, bufs, rows, stream)

    # ------------------------------------------------------------------------------- supersampled render
    def alloc_ss(self, width: int, height: int, rows: Optional[abi.rt_rows] = None, rgba32f=True, rgba8=False,
                 rgb64f=False, raycount=False):
        """Buffers of a supersampled render: as alloc(), but `raycount` holds two words per pixel, shape
        (rows, W, 2): primary + reflected segments and shadow rays, summed over the pixel's samples."""
        bufs = self.alloc(width, height, rows, rgba32f, rgba8, rgb64f, False)
        if raycount:
            nl = scenes.local_rows(height, rows)
            bufs["raycount"] = torch.empty((nl, width, 2), dtype=torch.int32, device=torch.device("cuda", self.device))
        return bufs

    def render_ss_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int, bufs: dict,
                       rows: Optional[abi.rt_rows] = None, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_ss_dev: samples x samples regular-grid samples per pixel summed in the kernel (samples in
        1, 2, 4, 8); asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_render_ss_dev(self._ctx, ctypes.byref(cam), width, height, depth, samples,
                                             ctypes.byref(rows) if rows is not None else None,
                                             _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")),
                                             _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")),
                                             ctypes.c_void_p(st.cuda_stream)), "rt_render_ss_dev")
        return bufs

    def render_ss(self, cam, width, height, depth, samples, rows=None, rgba32f=True, rgba8=False, rgb64f=False,
                  raycount=False, stream=None):
        bufs = self.alloc_ss(width, height, rows, rgba32f, rgba8, rgb64f, raycount)
        return self.render_ss_into(cam, width, height, depth, samples, bufs, rows, stream)

    # ---------------------------------------------------------------------------- adaptive supersampling
    def alloc_adaptive(self, width: int, height: int, samples: int, rgba32f=True, rgba8=False, rgb64f=False,
                       raycount=False, refined=True):
        """Buffers of an adaptive render (full frames): as alloc_ss(), plus `refined` (H, W) uint8 and the
        `workspace` byte tensor sized by rt_adaptive_workspace_bytes (one render at a time may use it)."""
        n = ctypes.c_size_t()
        abi.check(abi.lib().rt_adaptive_workspace_bytes(width, height, samples, ctypes.byref(n)),
                  "rt_adaptive_workspace_bytes")
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        dev = torch.device("cuda", self.device)
        bufs["refined"] = torch.empty((height, width), dtype=torch.uint8, device=dev) if refined else None
        bufs["workspace"] = torch.empty((n.value,), dtype=torch.uint8, device=dev)
        return bufs

    def render_adaptive_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int,
                             threshold: int, bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_adaptive_dev: samples x samples samples for the pixels whose base RGBA8 differs from a
        4-neighbour by more than `threshold` in some channel, one sample elsewhere; asynchronous on `stream`
        (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        ws = bufs.get("workspace")
        abi.check(abi.lib().rt_render_adaptive_dev(self._ctx, ctypes.byref(cam), width, height, depth, samples,
                                                   threshold, _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")),
                                                   _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")),
                                                   _ptr(bufs.get("refined")), _ptr(ws),
                                                   ws.numel() if ws is not None else 0,
                                                   ctypes.c_void_p(st.cuda_stream)), "rt_render_adaptive_dev")
        return bufs

    def render_adaptive(self, cam, width, height, depth, samples, threshold, rgba32f=True, rgba8=False,
                        rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_adaptive(), `refined` included."""
        bufs = self.alloc_adaptive(width, height, samples, rgba32f, rgba8, rgb64f, raycount)
        return self.render_adaptive_into(cam, width, height, depth, samples, threshold, bufs, stream)

    # ------------------------------------------------- the lens family: depth of field, soft shadows, motion blur
    def _render_lens_into(self, symbol: str, extra_floats, cam: abi.rt_camera, width: int, height: int, depth: int,
                          samples: int, bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """`symbol` (rt_render_dof_dev, rt_render_soft_dev or rt_render_motion_dev) into alloc_ss() buffers (full
        frames), `extra_floats` its doubles after `samples`; asynchronous on `stream` (default: torch's current
        stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(getattr(abi.lib(), symbol)(self._ctx, ctypes.byref(cam), width, height, depth, samples,
                                             *(float(v) for v in extra_floats), _ptr(bufs.get("rgba32f")),
                                             _ptr(bufs.get("rgba8")), _ptr(bufs.get("rgb64f")),
                                             _ptr(bufs.get("raycount")), ctypes.c_void_p(st.cuda_stream)), symbol)
        return bufs

    def render_dof_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int,
                        aperture: float, bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_dof_dev into alloc_ss() buffers (full frames): samples x samples rays per pixel from a square
        lens of half-width `aperture` around the eye, focused on the plane through cam.look_at
        (scenes.focus_camera moves it); asynchronous on `stream` (default: torch's current stream)."""
        return self._render_lens_into("rt_render_dof_dev", (aperture,), cam, width, height, depth, samples, bufs,
                                      stream)

    def render_dof(self, cam, width, height, depth, samples, aperture, rgba32f=True, rgba8=False, rgb64f=False,
                   raycount=False, stream=None):
        """-> the buffers of alloc_ss() (the keys of render_ss())."""
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        return self._render_lens_into("rt_render_dof_dev", (aperture,), cam, width, height, depth, samples, bufs,
                                      stream)

    def render_soft_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int,
                         aperture: float, light_size: float, bufs: dict,
                         stream: Optional[torch.cuda.Stream] = None):
        """rt_render_soft_dev into alloc_ss() buffers (full frames): the rays of render_dof_into(), sample (a, b)
        lit by point (a, b) of every light's square panel of half-width `light_size` in the world xz-plane;
        asynchronous on `stream` (default: torch's current stream)."""
        return self._render_lens_into("rt_render_soft_dev", (aperture, light_size), cam, width, height, depth, samples,
                                      bufs, stream)

    def render_soft(self, cam, width, height, depth, samples, aperture, light_size, rgba32f=True, rgba8=False,
                    rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_ss() (the keys of render_ss())."""
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        return self._render_lens_into("rt_render_soft_dev", (aperture, light_size), cam, width, height, depth, samples,
                                      bufs, stream)

    def set_motion(self, displacement=None):
        """rt_set_motion: `displacement` (n_spheres, 3), the half-extent of each sphere's motion during the exposure
        in scene-local coordinates; None clears the motion.  A changed set_scene() clears it too."""
        if displacement is None:
            abi.check(abi.lib().rt_set_motion(self._ctx, None, 0), "rt_set_motion")
            return
        flat = [float(v) for row in displacement for v in row]
        if len(flat) % 3:
            raise ValueError("set_motion: three components per sphere")
        d = (ctypes.c_double * max(len(flat), 1))(*flat)
        abi.check(abi.lib().rt_set_motion(self._ctx, d, len(flat) // 3), "rt_set_motion")

    def render_motion_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int,
                           aperture: float, light_size: float, shutter: float, bufs: dict,
                           stream: Optional[torch.cuda.Stream] = None):
        """rt_render_motion_dev into alloc_ss() buffers (full frames): the rays and lights of render_soft_into(),
        sample (a, b) at shutter time shutter * (2 (a + S b) + 1 - S S) / (S S) of the motion set_motion() gave;
        asynchronous on `stream` (default: torch's current stream)."""
        return self._render_lens_into("rt_render_motion_dev", (aperture, light_size, shutter), cam, width, height,
                                      depth, samples, bufs, stream)

    def render_motion(self, cam, width, height, depth, samples, aperture, light_size, shutter, rgba32f=True,
                      rgba8=False, rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_ss() (the keys of render_ss())."""
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        return self._render_lens_into("rt_render_motion_dev", (aperture, light_size, shutter), cam, width, height,
                                      depth, samples, bufs, stream)

    def render_jitter_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples: int, jitter: int,
                           seed: int, aperture: float, light_size: float, shutter: float, bufs: dict,
                           stream: Optional[torch.cuda.Stream] = None):
        """rt_render_jitter_dev into alloc_ss() buffers (full frames): the frame of render_motion_into() with every
        sample moved, in each of its seven dimensions (sub-pixel, lens, light, time), to one of `jitter` sub-positions
        of its stratum, chosen by a hash of the sample and `seed` (uint32); jitter = 1 is render_motion_into();
        asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_render_jitter_dev(
            self._ctx, ctypes.byref(cam), width, height, depth, samples, jitter, int(seed) & 0xFFFFFFFF,
            float(aperture), float(light_size), float(shutter), _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")),
            _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")), ctypes.c_void_p(st.cuda_stream)),
            "rt_render_jitter_dev")
        return bufs

    def render_jitter(self, cam, width, height, depth, samples, jitter, seed, aperture, light_size, shutter,
                      rgba32f=True, rgba8=False, rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_ss() (the keys of render_ss())."""
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        return self.render_jitter_into(cam, width, height, depth, samples, jitter, seed, aperture, light_size, shutter,
                                       bufs, stream)

    def render_shutter_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int, height: int,
                            depth: int, samples: int, jitter: int, seed: int, aperture: float, light_size: float,
                            shutter: float, bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_shutter_dev into alloc_ss() buffers (full frames): the frame of render_jitter_into() with the
        camera moving during the exposure: a sample at shutter time sigma sees from cam.eye + sigma * motion.eye
        towards cam.look_at + sigma * motion.look_at (scenes.camera_motion; None: a frozen camera, which is
        render_jitter_into()); asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_render_shutter_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height, depth,
            samples, jitter, int(seed) & 0xFFFFFFFF, float(aperture), float(light_size), float(shutter),
            _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")), _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")),
            ctypes.c_void_p(st.cuda_stream)), "rt_render_shutter_dev")
        return bufs

    def render_shutter(self, cam, motion, width, height, depth, samples, jitter, seed, aperture, light_size, shutter,
                       rgba32f=True, rgba8=False, rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_ss() (the keys of render_ss())."""
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        return self.render_shutter_into(cam, motion, width, height, depth, samples, jitter, seed, aperture, light_size,
                                        shutter, bufs, stream)

    # ---------------------------------------------------------------------------- progressive accumulation
    def alloc_accum(self, width: int, height: int):
        """The running sums of render_accum_into(): (H, W, 3) float64, uninitialised (a call with first_pass = 0 does
        not read them)."""
        return torch.empty((height, width, 3), dtype=torch.float64, device=torch.device("cuda", self.device))

    def render_accum_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int, height: int,
                          depth: int, samples: int, jitter: int, seed: int, first_pass: int, passes: int,
                          aperture: float, light_size: float, shutter: float, accum: torch.Tensor, bufs: dict,
                          stream: Optional[torch.cuda.Stream] = None):
        """rt_render_accum_dev: the frames render_shutter_into() gives the seeds seed + first_pass .. seed + first_pass
        + passes - 1 added to `accum` (alloc_accum()) one by one, in that order, and the mean of all first_pass + passes
        frames written into alloc_ss() buffers (`raycount`: the sums of this call's passes); first_pass = 0 starts a
        new sum.  Asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if accum is None or accum.dtype != torch.float64 or accum.numel() != width * height * 3:
            raise ValueError("accum must be a float64 tensor of width * height * 3 elements (alloc_accum)")
        abi.check(abi.lib().rt_render_accum_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height, depth,
            samples, jitter, int(seed) & 0xFFFFFFFF, int(first_pass), int(passes), float(aperture), float(light_size),
            float(shutter), _ptr(accum), _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")), _ptr(bufs.get("rgb64f")),
            _ptr(bufs.get("raycount")), ctypes.c_void_p(st.cuda_stream)), "rt_render_accum_dev")
        return bufs

    def render_accum(self, cam, motion, width, height, depth, samples, jitter, seed, first_pass, passes, aperture,
                     light_size, shutter, accum=None, rgba32f=True, rgba8=False, rgb64f=False, raycount=False,
                     stream=None):
        """-> (the buffers of alloc_ss(), the accumulator): `accum` continued, or a new one when it is None (then
        first_pass must be 0)."""
        if accum is None:
            if first_pass != 0:
                raise ValueError("first_pass > 0 continues a sum: pass its accum")
            accum = self.alloc_accum(width, height)
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        self.render_accum_into(cam, motion, width, height, depth, samples, jitter, seed, first_pass, passes, aperture,
                               light_size, shutter, accum, bufs, stream)
        return bufs, accum

    # ---------------------------------------------------------------------------- converging accumulation
    def alloc_converge(self, width: int, height: int):
        """The state of render_converge_into(): (accum, accum2, count) — two (H, W, 3) float64 tensors, uninitialised
        (a pixel with count 0 does not read them), and a zeroed (H, W) int32 tensor holding uint32 pass counts."""
        dev = torch.device("cuda", self.device)
        return (torch.empty((height, width, 3), dtype=torch.float64, device=dev),
                torch.empty((height, width, 3), dtype=torch.float64, device=dev),
                torch.zeros((height, width), dtype=torch.int32, device=dev))

    def render_converge_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int, height: int,
                             depth: int, samples: int, jitter: int, seed: int, passes: int, min_passes: int,
                             tolerance: float, aperture: float, light_size: float, shutter: float, state, bufs: dict,
                             active: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_converge_dev: up to `passes` more passes per pixel of the sum render_accum_into() forms, each pixel
        continuing from its own count in `state` (alloc_converge()) and stopping once it has `min_passes` passes and
        the estimated standard error of its mean is at most `tolerance` in every channel; the mean of every pixel's
        passes written into alloc_ss() buffers (`raycount`: the sums of this call's passes) and the number of pixels
        not yet stopped into `active` (a one-element int32 tensor, or None).  Asynchronous on `stream` (default:
        torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        accum, accum2, count = state
        for t, name in ((accum, "accum"), (accum2, "accum2")):
            if t is None or t.dtype != torch.float64 or t.numel() != width * height * 3:
                raise ValueError(f"{name} must be a float64 tensor of width * height * 3 elements (alloc_converge)")
        if count is None or count.dtype != torch.int32 or count.numel() != width * height:
            raise ValueError("count must be an int32 tensor of width * height elements (alloc_converge)")
        if active is not None and (active.dtype != torch.int32 or active.numel() != 1):
            raise ValueError("active must be a one-element int32 tensor")
        abi.check(abi.lib().rt_render_converge_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height, depth,
            samples, jitter, int(seed) & 0xFFFFFFFF, int(passes), int(min_passes) & 0xFFFFFFFF, float(tolerance),
            float(aperture), float(light_size), float(shutter), _ptr(accum), _ptr(accum2), _ptr(count),
            _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")), _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")),
            _ptr(active), ctypes.c_void_p(st.cuda_stream)), "rt_render_converge_dev")
        return bufs

    def render_converge(self, cam, motion, width, height, depth, samples, jitter, seed, passes, min_passes, tolerance,
                        aperture, light_size, shutter, state=None, rgba32f=True, rgba8=False, rgb64f=False,
                        raycount=False, stream=None):
        """-> (the buffers of alloc_ss(), the state, the active count as a one-element device tensor): `state`
        continued, or a new one when it is None."""
        if state is None:
            state = self.alloc_converge(width, height)
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        active = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", self.device))
        self.render_converge_into(cam, motion, width, height, depth, samples, jitter, seed, passes, min_passes,
                                  tolerance, aperture, light_size, shutter, state, bufs, active, stream)
        return bufs, state, active

    # ------------------------------------------------- windows of the accumulating and converging renders
    _WINDOW_BUFS = {"accum": (torch.float64, 3), "accum2": (torch.float64, 3), "count": (torch.int32, 1),
                    "rgba32f": (torch.float32, 4), "rgba8": (torch.uint8, 4), "rgb64f": (torch.float64, 3),
                    "raycount": (torch.int32, 2)}

    def _window(self, width: int, height: int, window, tensors: dict):
        """-> (rt_window, {name: pointer}).  Each tensor is a full-frame one, (height, width[, C]), in which the window
        lies in place, or one of the window's own (h, w[, C]) pixels — dense, or a view of wider rows; all must give
        the same row stride."""
        try:
            x0, y0, w, h = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError("window must be (x0, y0, width, height)") from None
        if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > width or y0 + h > height:
            raise ValueError(f"window {(x0, y0, w, h)} is empty or leaves the {width} x {height} frame")
        stride, ptrs = None, {}
        for name, t in tensors.items():
            if t is None:
                ptrs[name] = None
                continue
            dtype, c = self._WINDOW_BUFS[name]
            if not t.is_cuda or t.dtype != dtype:
                raise ValueError(f"{name} must be a HIP tensor of {dtype}")
            if t.dim() == 2 and c == 1:
                t = t.unsqueeze(-1)
            if t.dim() != 3 or t.shape[2] != c:
                raise ValueError(f"{name} must have {c} element(s) per pixel in its last dimension")
            if tuple(t.shape[:2]) == (height, width):
                t = t[y0:y0 + h, x0:x0 + w]
            elif tuple(t.shape[:2]) != (h, w):
                raise ValueError(f"{name} must hold the {height} x {width} frame or the {h} x {w} window, not "
                                 f"{tuple(t.shape[:2])}")
            if (c > 1 and t.stride(2) != 1) or t.stride(1) != c or t.stride(0) % c or t.stride(0) < w * c:
                raise ValueError(f"{name}: pixels must be contiguous within a row and rows a whole number of pixels apart")
            if stride is not None and t.stride(0) // c != stride:
                raise ValueError(f"{name}: every buffer of a window must have the same row stride in pixels")
            stride = t.stride(0) // c
            ptrs[name] = ctypes.c_void_p(t.data_ptr())
        return abi.rt_window(x0, y0, w, h, stride if stride is not None else w), ptrs

    def render_accum_window_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int,
                                 height: int, window, depth: int, samples: int, jitter: int, seed: int, first_pass: int,
                                 passes: int, aperture: float, light_size: float, shutter: float, accum: torch.Tensor,
                                 bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_accum_window_dev: render_accum_into() for the pixels of window = (x0, y0, w, h) of the width x
        height frame alone, with the full frame's bytes.  `accum` and every buffer of `bufs` is either a full-frame
        tensor, in which the window is rendered in place and nothing else is touched, or a tensor of the window's own
        h x w pixels.  Asynchronous on `stream` (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if accum is None:
            raise ValueError("accum is required")
        win, p = self._window(width, height, window, {"accum": accum, **{k: bufs.get(k) for k in
                                                                         ("rgba32f", "rgba8", "rgb64f", "raycount")}})
        abi.check(abi.lib().rt_render_accum_window_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height,
            ctypes.byref(win), depth, samples, jitter, int(seed) & 0xFFFFFFFF, int(first_pass), int(passes),
            float(aperture), float(light_size), float(shutter), p["accum"], p["rgba32f"], p["rgba8"], p["rgb64f"],
            p["raycount"], ctypes.c_void_p(st.cuda_stream)), "rt_render_accum_window_dev")
        return bufs

    def render_accum_window(self, cam, motion, width, height, window, depth, samples, jitter, seed, first_pass, passes,
                            aperture, light_size, shutter, accum=None, rgba32f=True, rgba8=False, rgb64f=False,
                            raycount=False, stream=None):
        """-> (dense buffers of the window's h x w pixels as alloc_ss() lays them out, the accumulator): `accum`
        continued (full-frame or dense), or a new dense one when it is None (then first_pass must be 0)."""
        _, _, w, h = window
        if accum is None:
            if first_pass != 0:
                raise ValueError("first_pass > 0 continues a sum: pass its accum")
            accum = self.alloc_accum(w, h)
        bufs = self.alloc_ss(w, h, None, rgba32f, rgba8, rgb64f, raycount)
        self.render_accum_window_into(cam, motion, width, height, window, depth, samples, jitter, seed, first_pass,
                                      passes, aperture, light_size, shutter, accum, bufs, stream)
        return bufs, accum

    def render_converge_window_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int,
                                    height: int, window, depth: int, samples: int, jitter: int, seed: int, passes: int,
                                    min_passes: int, tolerance: float, aperture: float, light_size: float,
                                    shutter: float, state, bufs: dict, active: Optional[torch.Tensor] = None,
                                    stream: Optional[torch.cuda.Stream] = None):
        """rt_render_converge_window_dev: render_converge_into() for the pixels of window = (x0, y0, w, h) alone, with
        the full frame's bytes; `active` counts the window's pixels.  The three tensors of `state` and every buffer of
        `bufs` are full-frame tensors (the window in place) or tensors of the window's h x w pixels."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        accum, accum2, count = state
        if accum is None or accum2 is None or count is None:
            raise ValueError("state must be (accum, accum2, count)")
        if active is not None and (active.dtype != torch.int32 or active.numel() != 1):
            raise ValueError("active must be a one-element int32 tensor")
        win, p = self._window(width, height, window, {"accum": accum, "accum2": accum2, "count": count,
                                                      **{k: bufs.get(k) for k in
                                                         ("rgba32f", "rgba8", "rgb64f", "raycount")}})
        abi.check(abi.lib().rt_render_converge_window_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height,
            ctypes.byref(win), depth, samples, jitter, int(seed) & 0xFFFFFFFF, int(passes),
            int(min_passes) & 0xFFFFFFFF, float(tolerance), float(aperture), float(light_size), float(shutter),
            p["accum"], p["accum2"], p["count"], p["rgba32f"], p["rgba8"], p["rgb64f"], p["raycount"], _ptr(active),
            ctypes.c_void_p(st.cuda_stream)), "rt_render_converge_window_dev")
        return bufs

    def render_converge_window(self, cam, motion, width, height, window, depth, samples, jitter, seed, passes,
                               min_passes, tolerance, aperture, light_size, shutter, state=None, rgba32f=True,
                               rgba8=False, rgb64f=False, raycount=False, stream=None):
        """-> (dense buffers of the window's pixels, the state, the window's active count as a one-element device
        tensor): `state` continued (full-frame or dense), or a new dense one when it is None."""
        _, _, w, h = window
        if state is None:
            state = self.alloc_converge(w, h)
        bufs = self.alloc_ss(w, h, None, rgba32f, rgba8, rgb64f, raycount)
        active = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", self.device))
        self.render_converge_window_into(cam, motion, width, height, window, depth, samples, jitter, seed, passes,
                                         min_passes, tolerance, aperture, light_size, shutter, state, bufs, active,
                                         stream)
        return bufs, state, active

    # --------------------------------------- lists of windows of the accumulating and converging renders
    _LAYOUTS = {"inplace": abi.RT_WINDOWS_IN_PLACE, "packed": abi.RT_WINDOWS_PACKED}

    def set_windows(self, width: int, height: int, windows, layout: str = "inplace"):
        """rt_set_windows: the list of disjoint windows (x0, y0, w, h) of the width x height frame the list renders
        below draw, and how their buffers are laid out: "inplace" (full-frame buffers) or "packed" (every window dense,
        one after the other in list order, in flat buffers).  windows = None clears the list.  Synchronous.  -> the
        number of per-pixel elements a buffer must hold (0 for a cleared list).  The Tracer remembers the list's
        frame, layout and elements for its buffer checks: a list set on the same context behind its back (the C host
        conveniences rt_render_*_windows) is not seen by them — set lists through this method."""
        if windows is None:
            abi.check(abi.lib().rt_set_windows(self._ctx, 0, 0, None, 0, 0), "rt_set_windows")
            self._windows = None
            return 0
        if layout not in self._LAYOUTS:
            raise ValueError('layout must be "inplace" or "packed"')
        try:
            wins = [tuple(int(v) for v in w) for w in windows]
            arr = (abi.rt_window * max(len(wins), 1))(*[abi.rt_window(x0, y0, w, h, 0) for x0, y0, w, h in wins])
        except (TypeError, ValueError):
            raise ValueError("windows must be a sequence of (x0, y0, width, height)") from None
        # (rt_set_windows validates the list itself: no rt_window_list_plan call, whose disjointness check it repeats)
        abi.check(abi.lib().rt_set_windows(self._ctx, width, height, arr, len(wins), self._LAYOUTS[layout]),
                  "rt_set_windows")
        elements = sum(w * h for _, _, w, h in wins) if layout == "packed" else width * height
        self._windows = (width, height, layout, elements)
        return elements

    def _windows_shape(self, c: int):
        """The shape of a C-channel buffer of the list in force: the full frame's in place, (elements[, C]) packed."""
        if self._windows is None:
            raise ValueError("no list of windows set (set_windows)")
        width, height, layout, elements = self._windows
        lead = (elements,) if layout == "packed" else (height, width)
        return lead + ((c,) if c > 1 else ())

    def alloc_windows(self, rgba32f=True, rgba8=False, rgb64f=False, raycount=False):
        """The output buffers of a list render, as alloc_ss() gives them for a frame, laid out for the list in force:
        full-frame tensors in place, flat (elements, C) tensors packed.  Uninitialised."""
        dev = torch.device("cuda", self.device)
        bufs = {}
        for name, want in (("rgba32f", rgba32f), ("rgba8", rgba8), ("rgb64f", rgb64f), ("raycount", raycount)):
            if want:
                dtype, c = self._WINDOW_BUFS[name]
                bufs[name] = torch.empty(self._windows_shape(c), dtype=dtype, device=dev)
        return bufs

    def alloc_windows_accum(self):
        """The running sums of render_accum_windows_into() for the list in force, uninitialised."""
        return torch.empty(self._windows_shape(3), dtype=torch.float64, device=torch.device("cuda", self.device))

    def alloc_windows_converge(self):
        """The state (accum, accum2, count) of render_converge_windows_into() for the list in force; count zeroed."""
        dev = torch.device("cuda", self.device)
        return (torch.empty(self._windows_shape(3), dtype=torch.float64, device=dev),
                torch.empty(self._windows_shape(3), dtype=torch.float64, device=dev),
                torch.zeros(self._windows_shape(1), dtype=torch.int32, device=dev))

    def _windows_ptrs(self, width: int, height: int, tensors: dict):
        """{name: pointer} of the buffers of a list render, each checked to be a contiguous HIP tensor of its type with
        at least the elements the list in force needs."""
        if self._windows is None:
            raise ValueError("no list of windows set (set_windows)")
        if (width, height) != self._windows[:2]:
            raise ValueError(f"the list of windows is of the {self._windows[0]} x {self._windows[1]} frame")
        ptrs = {}
        for name, t in tensors.items():
            if t is None:
                ptrs[name] = None
                continue
            dtype, c = self._WINDOW_BUFS[name]
            if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < self._windows[3] * c:
                raise ValueError(f"{name} must be a contiguous HIP tensor of {dtype} holding {self._windows[3]} "
                                 f"elements of {c} (alloc_windows)")
            ptrs[name] = ctypes.c_void_p(t.data_ptr())
        return ptrs

    def render_accum_windows_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int,
                                  height: int, depth: int, samples: int, jitter: int, seed: int, first_pass: int,
                                  passes: int, aperture: float, light_size: float, shutter: float, accum: torch.Tensor,
                                  bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_accum_windows_dev: render_accum_into() for the pixels of every window of the list in force
        (set_windows) in one launch per launch group, with the full frame's bytes; nothing else of the buffers
        (alloc_windows_accum(), alloc_windows()) is touched.  Asynchronous on `stream` (default: torch's current
        stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if accum is None:
            raise ValueError("accum is required")
        p = self._windows_ptrs(width, height, {"accum": accum, **{k: bufs.get(k) for k in
                                                                  ("rgba32f", "rgba8", "rgb64f", "raycount")}})
        abi.check(abi.lib().rt_render_accum_windows_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height, depth,
            samples, jitter, int(seed) & 0xFFFFFFFF, int(first_pass), int(passes), float(aperture), float(light_size),
            float(shutter), p["accum"], p["rgba32f"], p["rgba8"], p["rgb64f"], p["raycount"],
            ctypes.c_void_p(st.cuda_stream)), "rt_render_accum_windows_dev")
        return bufs

    def render_accum_windows(self, cam, motion, width, height, depth, samples, jitter, seed, first_pass, passes,
                             aperture, light_size, shutter, accum=None, rgba32f=True, rgba8=False, rgb64f=False,
                             raycount=False, stream=None):
        """-> (the buffers of alloc_windows(), the accumulator): `accum` continued, or a new one when it is None (then
        first_pass must be 0)."""
        if accum is None:
            if first_pass != 0:
                raise ValueError("first_pass > 0 continues a sum: pass its accum")
            accum = self.alloc_windows_accum()
        bufs = self.alloc_windows(rgba32f, rgba8, rgb64f, raycount)
        self.render_accum_windows_into(cam, motion, width, height, depth, samples, jitter, seed, first_pass, passes,
                                       aperture, light_size, shutter, accum, bufs, stream)
        return bufs, accum

    def render_converge_windows_into(self, cam: abi.rt_camera, motion: Optional[abi.rt_camera_motion], width: int,
                                     height: int, depth: int, samples: int, jitter: int, seed: int, passes: int,
                                     min_passes: int, tolerance: float, aperture: float, light_size: float,
                                     shutter: float, state, bufs: dict, active: Optional[torch.Tensor] = None,
                                     stream: Optional[torch.cuda.Stream] = None):
        """rt_render_converge_windows_dev: render_converge_into() for the pixels of every window of the list in force in
        one launch per launch group, with the full frame's bytes; `active` counts the list's pixels."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        accum, accum2, count = state
        if accum is None or accum2 is None or count is None:
            raise ValueError("state must be (accum, accum2, count)")
        if active is not None and (active.dtype != torch.int32 or active.numel() != 1):
            raise ValueError("active must be a one-element int32 tensor")
        p = self._windows_ptrs(width, height, {"accum": accum, "accum2": accum2, "count": count,
                                               **{k: bufs.get(k) for k in ("rgba32f", "rgba8", "rgb64f", "raycount")}})
        abi.check(abi.lib().rt_render_converge_windows_dev(
            self._ctx, ctypes.byref(cam), ctypes.byref(motion) if motion is not None else None, width, height, depth,
            samples, jitter, int(seed) & 0xFFFFFFFF, int(passes), int(min_passes) & 0xFFFFFFFF, float(tolerance),
            float(aperture), float(light_size), float(shutter), p["accum"], p["accum2"], p["count"], p["rgba32f"],
            p["rgba8"], p["rgb64f"], p["raycount"], _ptr(active), ctypes.c_void_p(st.cuda_stream)),
            "rt_render_converge_windows_dev")
        return bufs

    def render_converge_windows(self, cam, motion, width, height, depth, samples, jitter, seed, passes, min_passes,
                                tolerance, aperture, light_size, shutter, state=None, rgba32f=True, rgba8=False,
                                rgb64f=False, raycount=False, stream=None):
        """-> (the buffers of alloc_windows(), the state, the list's active count as a one-element device tensor):
        `state` continued, or a new one when it is None."""
        if state is None:
            state = self.alloc_windows_converge()
        bufs = self.alloc_windows(rgba32f, rgba8, rgb64f, raycount)
        active = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", self.device))
        self.render_converge_windows_into(cam, motion, width, height, depth, samples, jitter, seed, passes, min_passes,
                                          tolerance, aperture, light_size, shutter, state, bufs, active, stream)
        return bufs, state, active

    # ------------------------------------------------------------ adaptive sampling of the lens family's renders
    def alloc_lens_adaptive(self, width: int, height: int, rgba32f=True, rgba8=False, rgb64f=False, raycount=False,
                            refined=True):
        """Buffers of an adaptive lens render (full frames): as alloc_ss(), plus `refined` (H, W) uint8 and the
        `workspace` byte tensor sized by rt_lens_adaptive_workspace_bytes (one render at a time may use it)."""
        n = ctypes.c_size_t()
        abi.check(abi.lib().rt_lens_adaptive_workspace_bytes(width, height, ctypes.byref(n)),
                  "rt_lens_adaptive_workspace_bytes")
        bufs = self.alloc_ss(width, height, None, rgba32f, rgba8, rgb64f, raycount)
        dev = torch.device("cuda", self.device)
        bufs["refined"] = torch.empty((height, width), dtype=torch.uint8, device=dev) if refined else None
        bufs["workspace"] = torch.empty((n.value,), dtype=torch.uint8, device=dev)
        return bufs

    def render_lens_adaptive_into(self, cam: abi.rt_camera, width: int, height: int, depth: int, samples_lo: int,
                                  samples_hi: int, threshold: int, aperture: float, light_size: float,
                                  shutter: float, bufs: dict, stream: Optional[torch.cuda.Stream] = None):
        """rt_render_lens_adaptive_dev: the frame of render_motion_into() with samples_lo x samples_lo samples per
        pixel, and samples_hi x samples_hi for the pixels whose coarse samples' RGBA8 bytes spread by more than
        `threshold` or whose coarse RGBA8 differs from a 4-neighbour by more than it; asynchronous on `stream`
        (default: torch's current stream)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        ws = bufs.get("workspace")
        abi.check(abi.lib().rt_render_lens_adaptive_dev(
            self._ctx, ctypes.byref(cam), width, height, depth, samples_lo, samples_hi, threshold, float(aperture),
            float(light_size), float(shutter), _ptr(bufs.get("rgba32f")), _ptr(bufs.get("rgba8")),
            _ptr(bufs.get("rgb64f")), _ptr(bufs.get("raycount")), _ptr(bufs.get("refined")), _ptr(ws),
            ws.numel() if ws is not None else 0, ctypes.c_void_p(st.cuda_stream)), "rt_render_lens_adaptive_dev")
        return bufs

    def render_lens_adaptive(self, cam, width, height, depth, samples_lo, samples_hi, threshold, aperture, light_size,
                             shutter, rgba32f=True, rgba8=False, rgb64f=False, raycount=False, stream=None):
        """-> the buffers of alloc_lens_adaptive(), `refined` included."""
        bufs = self.alloc_lens_adaptive(width, height, rgba32f, rgba8, rgb64f, raycount)
        return self.render_lens_adaptive_into(cam, width, height, depth, samples_lo, samples_hi, threshold, aperture,
                                              light_size, shutter, bufs, stream)

    def render_packed(self, cam, width, height, depth, float_format=None, byte_format=None, rows=None,
                      stream=None):
        """rt_render_dev_packed: the float image in float_format (RT_PIXEL_RGBA32F / GRAY32F) and the byte
        image in byte_format (RT_PIXEL_RGBA8 / RGB8 / GRAY8), each None to skip.  Returns (float, byte)
        tensors of shape (rows, W, channels)."""
        nl = scenes.local_rows(height, rows)
        dev = torch.device("cuda", self.device)
        ch = {abi.RT_PIXEL_RGBA32F: 4, abi.RT_PIXEL_GRAY32F: 1, abi.RT_PIXEL_RGBA8: 4, abi.RT_PIXEL_RGB8: 3,
              abi.RT_PIXEL_GRAY8: 1}
        f = torch.empty((nl, width, ch[float_format]), dtype=torch.float32, device=dev) if float_format is not None \
            else None
        b = torch.empty((nl, width, ch[byte_format]), dtype=torch.uint8, device=dev) if byte_format is not None \
            else None
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_render_dev_packed(
            self._ctx, ctypes.byref(cam), width, height, depth, ctypes.byref(rows) if rows is not None else None,
            float_format if float_format is not None else abi.RT_PIXEL_RGBA32F, _ptr(f),
            byte_format if byte_format is not None else abi.RT_PIXEL_RGBA8, _ptr(b),
            ctypes.c_void_p(st.cuda_stream)), "rt_render_dev_packed")
        return f, b

    def render_host(self, scene_abi, cam, width, height, depth, rows=None):
        """rt_render (host buffers, synchronous) -> (rgb64f numpy, rt_stats)."""
        import numpy as np
        nl = scenes.local_rows(height, rows)
        rgb = np.zeros((nl, width, 3), np.float64)
        st = abi.rt_stats()
        abi.check(abi.lib().rt_render(self._ctx, ctypes.byref(scene_abi), ctypes.byref(cam), width, height, depth,
                                      ctypes.byref(rows) if rows is not None else None, None, None,
                                      ctypes.c_void_p(rgb.ctypes.data), ctypes.byref(st)), "rt_render")
        return rgb, st

    # ------------------------------------------------------------------------------------ ray lists
    def trace_rays(self, starts: torch.Tensor, ends: torch.Tensor, depth: int, stream=None):
        n = starts.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float64, device=starts.device)
        rc = torch.empty((n,), dtype=torch.int32, device=starts.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_trace_rays_dev(self._ctx, _ptr(starts), _ptr(ends), n, depth, _ptr(rgb), _ptr(rc),
                                              ctypes.c_void_p(st.cuda_stream)), "rt_trace_rays_dev")
        return rgb, rc

    def intersect(self, starts: torch.Tensor, ends: torch.Tensor, stream=None):
        n = starts.shape[0]
        raw = torch.empty((n, ctypes.sizeof(abi.rt_hit)), dtype=torch.uint8, device=starts.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        abi.check(abi.lib().rt_intersect_dev(self._ctx, _ptr(starts), _ptr(ends), n, _ptr(raw),
                                             ctypes.c_void_p(st.cuda_stream)), "rt_intersect_dev")
        return raw


def unshuffle(gathered: torch.Tensor, image: torch.Tensor, width: int, height: int, band_height: int,
              n_ranks: int, slab_rows: int, stream=None):
    """rt_unshuffle_dev: gathered [n_ranks, slab_rows, W, C] -> image [H, W, C] (same dtype)."""
    elem = gathered.element_size() * (gathered.shape[-1] if gathered.dim() == 4 else 1)
    st = stream if stream is not None else torch.cuda.current_stream(image.device)
    abi.check(abi.lib().rt_unshuffle_dev(_ptr(gathered), _ptr(image), width, height, elem, band_height, n_ranks,
                                         slab_rows, ctypes.c_void_p(st.cuda_stream)), "rt_unshuffle_dev")
    return image


def unpack(gathered: torch.Tensor, image: torch.Tensor, width: int, height: int, src_format: int, dst_format: int,
           band_height: int, n_ranks: int, slab_rows: int, stream=None):
    """rt_unpack_dev: packed slabs (src_format) -> image (dst_format), bands put in image order."""
    st = stream if stream is not None else torch.cuda.current_stream(image.device)
    abi.check(abi.lib().rt_unpack_dev(_ptr(gathered), _ptr(image), width, height, src_format, dst_format, band_height,
                                      n_ranks, slab_rows, ctypes.c_void_p(st.cuda_stream)), "rt_unpack_dev")
    return image


def decode_hits(raw: torch.Tensor) -> dict:
    """rt_hit records (bytes) -> dict of numpy arrays (host)."""
    import numpy as np
    a = raw.cpu().numpy()
    n = a.shape[0]
    d = a[:, :96].copy().view(np.float64).reshape(n, 12)
    i = a[:, 96:104].copy().view(np.int32).reshape(n, 2)
    return {"point": d[:, 0:3], "normal": d[:, 3:6], "reflected_end": d[:, 6:9], "transmitted_end": d[:, 9:12],
            "hit": i[:, 0], "material": i[:, 1]}
