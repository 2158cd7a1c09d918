"""The weights of all levels of one weighted multilevel solve, resident on the device (include/dotsocp.h:
dotsocp_weights_*, csrc/weights.hip): filled once at the finest level, restricted level by level on the GPU
(downSample_q.m / downSample_barrier.m) and handed to each level's context device to device."""
import ctypes

import numpy as np

from . import capi
from .examples import SpaceWeight


def weights_len(ny, nx, nt, levels, level):
    """Nq of level `level` of a pyramid whose finest level (levels - 1) is ny x nx x nt; -1 for a bad level or a grid that
    cannot be halved that often.  No device needed."""
    return int(capi.lib().dotsocp_weights_len(int(ny), int(nx), int(nt), int(levels), int(level)))


class WeightPyramid:
    """Level levels-1 is the finest grid ny x nx x nt; level l-1 has (n+1)/2 points per axis of level l."""

    def __init__(self, ny, nx, nt, levels, device=0):
        L = capi.lib()
        self.ny, self.nx, self.nt, self.levels = int(ny), int(nx), int(nt), int(levels)
        self._w = L.dotsocp_weights_create(int(device), self.ny, self.nx, self.nt, self.levels)
        if not self._w:
            # create returns NULL + last_error; the code follows the order of its checks: arguments, device, allocation
            msg = L.dotsocp_last_error().decode()
            ndev = L.dotsocp_device_count()
            if weights_len(ny, nx, nt, levels, 0) < 0:
                code = -1                                    # DOTSOCP_EINVAL: the grid / level arguments
            elif ndev == 0:
                code = -2                                    # DOTSOCP_ENODEVICE
            elif not 0 <= int(device) < ndev:
                code = -1                                    # the device ordinal
            else:
                code = -3                                    # DOTSOCP_EHIP: stream creation or an allocation failed
            raise capi.DotsocpError(code, msg)

    def len(self, level):
        return weights_len(self.ny, self.nx, self.nt, self.levels, level)

    def set(self, weight):
        """Finest level from the Nq array [q0; bx; by], or from a SpaceWeight (its two 2-D arrays are all that is uploaded)"""
        L = capi.lib()
        if isinstance(weight, SpaceWeight):
            if (weight.ny, weight.nx) != (self.ny, self.nx):
                raise ValueError("SpaceWeight of another grid")
            capi.check(L.dotsocp_weights_set_space(self._w, capi.fptr(weight.weightX), capi.fptr(weight.weightY)))
            return
        a = np.ascontiguousarray(weight, dtype=np.float64).ravel()
        if a.size != self.len(self.levels - 1):
            raise ValueError("weight must hold Nq entries of the finest level")
        capi.check(L.dotsocp_weights_set(self._w, capi.fptr(a)))

    def restrict(self, log_mean=False):
        """Levels levels-2 .. 0: downSample_q.m, or with log_mean downSample_barrier.m"""
        capi.check(capi.lib().dotsocp_weights_restrict(self._w, int(bool(log_mean))))

    def log10_mean(self, level):
        """mean(log10(weight + 1e-10)) of a level (solver_wdotsocp2d.m:312-316)"""
        m = capi.dbl()
        capi.check(capi.lib().dotsocp_weights_log10_mean(self._w, int(level), ctypes.byref(m)))
        return m.value

    def download(self, level):
        n = self.len(level)
        if n < 0:
            raise capi.DotsocpError(-1, "weight pyramid: level out of range")
        out = np.empty(n, dtype=np.float64)
        capi.check(capi.lib().dotsocp_weights_download(self._w, int(level), capi.fptr(out)))
        return out

    def upload_to(self, ctx, level):
        """model.weight of the context (an InPALMContext or a raw dotsocp_ctx pointer) <- level `level`"""
        capi.check(capi.lib().dotsocp_upload_weight_from(getattr(ctx, "_ctx", ctx), self._w, int(level)))

    def close(self):
        if getattr(self, "_w", None):
            capi.lib().dotsocp_weights_destroy(self._w)
            self._w = None

    def __del__(self):
        self.close()
