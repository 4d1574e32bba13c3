"""The noise model between two rounds: Optimiser::allReduceSigma
(src/Optimiser.cpp:6395-6709), normCorrection (:6201-6393), initSigma
(:5145-5243) and allocPreCal's sigRcpP rows (:8060-8071) over the kernels of
csrc/noise.hip.

    nm = noise.NoiseModel(stack.N, n_group, device)
    nm.init_from(stack)                                   # the first _sigRcp
    sig = nm.sig_rcp_rows(px, group)                      # -> Expectation.run
    ...                                                   # expectation + insert
    nm.norm_correction(stack, vol, quat, trans, r_l=rL, r_norm=rNorm)
    nm.update(stack, vol, quat, trans, offS=off, group=group)

Pose source: one pose per image from the caller (quat [n, 4] or 2D rot
[n, 2], trans [n, 2], dF [n], cls [n]).  The reference uses
Particle::rank1st: that is ``Expectation.rank1st()`` -- (cls, quat, trans, d,
vari), read right after the run; in 2D pass ``quat[:, :2].contiguous()``.

The sums over the hemisphere's images are all-reduced with
``hemisphere_group`` (a torch.distributed group), as stdN is in ingest.Stack.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import check, lib
from .ops import _ptr, _req, _stream

_vp = ctypes.c_void_p


def _np_ptr(a):
    return a.ctypes.data_as(_vp)


class SpectrumPixels:
    """thx_spectrum_pixels: powerSpectrum's pixels (src/Functions/Spectrum.cpp:
    161-190) shell by shell; shell u is [shellStart[u], shellStart[u+1])."""

    def __init__(self, idim, r, device=None):
        n = ctypes.c_int(0)
        start = np.zeros(max(r, 0) + 1, np.int32)
        check(lib().thx_spectrum_pixels(idim, r, 0, None, None, None, None, _np_ptr(start),
                                        ctypes.byref(n)), "thx_spectrum_pixels")
        n = n.value
        bufs = [np.zeros(n, np.int32) for _ in range(4)]
        check(lib().thx_spectrum_pixels(idim, r, n, *[_np_ptr(b) for b in bufs], _np_ptr(start),
                                        ctypes.byref(ctypes.c_int(0))), "thx_spectrum_pixels")
        self.idim, self.r, self.n = idim, r, n
        self.iCol, self.iRow, self.iShell, self.iPxl = bufs
        self.shellStart = start
        self.count = np.diff(start)
        self.device = device
        if device is not None:
            self.d_iCol, self.d_iRow, self.d_iPxl, self.d_shellStart = (
                torch.from_numpy(a).to(device) for a in (self.iCol, self.iRow, self.iPxl, start))


def _stack_dims(ft, name):
    if ft.dim() != 3 or ft.shape[2] != ft.shape[1] // 2 + 1:
        raise ValueError(f"{name}: expected [n, N, N/2+1] half-complex, got {tuple(ft.shape)}")
    _req(ft, torch.complex64, None, name)
    return ft.shape[0], ft.shape[1]


def power_spectrum(ft, sp):
    """thx_power_spectrum: [n, r] float32 shell means of |ft|^2."""
    n, N = _stack_dims(ft, "imgFT")
    if N != sp.idim:
        raise ValueError("pixel table / image size mismatch")
    out = torch.empty(n, sp.r, dtype=torch.float32, device=ft.device)
    check(lib().thx_power_spectrum(_ptr(ft), n, N, sp.r, _ptr(sp.d_iPxl), _ptr(sp.d_shellStart),
                                   _ptr(out), _stream(ft.device)), "thx_power_spectrum")
    return out


def residual_spectra(vol, imgFT, oriFT, attr, rot, trans, sp, pf=2, offS=None, dF=None, cls=None,
                     norm_radii=None):
    """thx_residual_spectra (rot [n, 4] quaternions, vol [nK, vdim, vdim,
    vdim/2+1] or one volume) or thx_residual_spectra2d (rot [n, 2], vol
    [nK, vdim, vdim/2+1]).  Returns (spectra [n, 4, r] float32 -- rows
    |img-M|^2, |ori-N|^2, |M|^2, |img|^2, row 1 zero without oriFT -- and
    norm [n] float64, or None without norm_radii = (rL, rNorm))."""
    n, N = _stack_dims(imgFT, "imgFT")
    dev = imgFT.device
    two_d = rot.shape[-1] == 2
    _req(vol, torch.complex64, None, "vol")
    if vol.dim() == (2 if two_d else 3):
        vol = vol.unsqueeze(0)
    vdim = vol.shape[1]
    want = (vol.shape[0], vdim, vdim // 2 + 1) if two_d else (vol.shape[0], vdim, vdim,
                                                              vdim // 2 + 1)
    if tuple(vol.shape) != want:
        raise ValueError(f"vol: expected {want}, got {tuple(vol.shape)}")
    if N != sp.idim:
        raise ValueError("pixel table / image size mismatch")
    if oriFT is not None:
        _req(oriFT, torch.complex64, tuple(imgFT.shape), "oriFT")
    _req(attr, torch.float32, (n, 8), "attr")
    _req(rot, torch.float64, (n, 2 if two_d else 4), "rot")
    _req(trans, torch.float64, (n, 2), "trans")
    if offS is not None:
        _req(offS, torch.float64, (n, 2), "offS")
    if dF is not None:
        _req(dF, torch.float64, (n,), "dF")
    if cls is not None:
        _req(cls, torch.int32, (n,), "cls")
    spectra = torch.zeros(n, 4, sp.r, dtype=torch.float32, device=dev)
    norm = torch.empty(n, dtype=torch.float64, device=dev) if norm_radii is not None else None
    rL, rN = norm_radii if norm_radii is not None else (0.0, 0.0)
    fn = lib().thx_residual_spectra2d if two_d else lib().thx_residual_spectra
    check(fn(_ptr(vol), vdim, pf, vol.shape[0], _ptr(imgFT), _ptr(oriFT), _ptr(attr), _ptr(rot),
             _ptr(trans), _ptr(offS), _ptr(dF), _ptr(cls), n, N, sp.r, _ptr(sp.d_iCol),
             _ptr(sp.d_iRow), _ptr(sp.d_iPxl), _ptr(sp.d_shellStart), _ptr(spectra), _ptr(norm),
             float(rL), float(rN), _stream(dev)),
          "thx_residual_spectra2d" if two_d else "thx_residual_spectra")
    return spectra, norm


def sigma_accumulate(spectra, group, n_group, acc=None):
    """thx_sigma_accumulate into acc [3, nGroup, r+1] float64 (created zeroed
    when None; never cleared).  group: [n] int32, 0-based, or None."""
    n, _, r = spectra.shape
    _req(spectra, torch.float32, (n, 4, r), "spectra")
    if group is not None:
        _req(group, torch.int32, (n,), "group")
    if acc is None:
        acc = torch.zeros(3, n_group, r + 1, dtype=torch.float64, device=spectra.device)
    _req(acc, torch.float64, (3, n_group, r + 1), "acc")
    check(lib().thx_sigma_accumulate(_ptr(spectra), _ptr(group), n, r, n_group, _ptr(acc),
                                     _stream(spectra.device)), "thx_sigma_accumulate")
    return acc


def sigma_finalise(acc, n_col, alpha, grouped):
    """thx_sigma_finalise on the (all-reduced) sums: (sig, sigRcp) float64
    numpy [nGroup, nCol]."""
    a = np.ascontiguousarray(acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else acc,
                             np.float64)
    _, n_group, r1 = a.shape
    sig = np.zeros((n_group, n_col), np.float64)
    rcp = np.zeros_like(sig)
    check(lib().thx_sigma_finalise(_np_ptr(a), n_group, r1 - 1, n_col, float(alpha),
                                   int(bool(grouped)), _np_ptr(sig), _np_ptr(rcp)),
          "thx_sigma_finalise")
    return sig, rcp


def sigma_init_accumulate(oriFT, sp, avg_sum=None, ps_sum=None):
    """thx_sigma_init_accumulate: (avgSum [N, N/2+1, 2], psSum [r]) float64."""
    n, N = _stack_dims(oriFT, "oriFT")
    dev = oriFT.device
    if avg_sum is None:
        avg_sum = torch.zeros(N, N // 2 + 1, 2, dtype=torch.float64, device=dev)
    if ps_sum is None:
        ps_sum = torch.zeros(sp.r, dtype=torch.float64, device=dev)
    _req(avg_sum, torch.float64, (N, N // 2 + 1, 2), "avgSum")
    _req(ps_sum, torch.float64, (sp.r,), "psSum")
    check(lib().thx_sigma_init_accumulate(_ptr(oriFT), n, N, sp.r, _ptr(sp.d_iPxl),
                                          _ptr(sp.d_shellStart), _ptr(avg_sum), _ptr(ps_sum),
                                          _stream(dev)), "thx_sigma_init_accumulate")
    return avg_sum, ps_sum


def sigma_init_finalise(avg_sum, ps_sum, n_total, idim, n_group, n_col):
    a = np.ascontiguousarray(avg_sum, np.float64)
    p = np.ascontiguousarray(ps_sum, np.float64)
    sig = np.zeros((n_group, n_col), np.float64)
    rcp = np.zeros_like(sig)
    check(lib().thx_sigma_init_finalise(_np_ptr(a), _np_ptr(p), float(n_total), idim, len(p),
                                        n_group, n_col, _np_ptr(sig), _np_ptr(rcp)),
          "thx_sigma_init_finalise")
    return sig, rcp


def img_scale(imgFT, oriFT, scale):
    """thx_img_scale in place: image l (and its oriFT) times scale[l]."""
    n, N = _stack_dims(imgFT, "imgFT")
    if oriFT is not None:
        _req(oriFT, torch.complex64, tuple(imgFT.shape), "oriFT")
    _req(scale, torch.float32, (n,), "scale")
    for l0 in range(0, n, 65535):
        nb = min(65535, n - l0)
        check(lib().thx_img_scale(_ptr(imgFT[l0:]), _ptr(oriFT[l0:]) if oriFT is not None else None,
                                  _ptr(scale[l0:]), nb, N, _stream(imgFT.device)), "thx_img_scale")


def _all_reduce(t, group):
    if group is None:
        return t
    import torch.distributed as dist
    st = t.cpu() if dist.get_backend(group) == "gloo" else t
    dist.all_reduce(st, group=group)
    return st.to(t.device)


class NoiseModel:
    """_sig / _sigRcp [nGroup, nCol] (float64; numpy on the host, sig_rcp_d on
    the device) of one hemisphere, nCol = maxR + 1 with maxR = N/2 - 1
    (SIGMA_WHOLE_FREQUENCY: the spectra always run to r = maxR)."""

    def __init__(self, idim, n_group, device, r=None, n_col=None):
        self.idim, self.n_group, self.device = idim, n_group, torch.device(device)
        self.r = idim // 2 - 1 if r is None else r
        self.n_col = self.r + 1 if n_col is None else n_col
        self.sp = SpectrumPixels(idim, self.r, self.device)
        self.sig = self.sig_rcp = self.sig_rcp_d = None
        self.acc = None            # the last update's all-reduced sums

    def _set(self, sig, rcp):
        self.sig, self.sig_rcp = sig, rcp
        self.sig_rcp_d = torch.from_numpy(rcp).to(self.device)

    def init_from(self, stack, hemisphere_group=None):
        """initSigma from stack.oriFT; returns (sig, sigRcp)."""
        if stack.oriFT is None:
            raise ValueError("init_from needs the unmasked oriFT (Stack(keep_ori=True))")
        avg, ps = sigma_init_accumulate(stack.oriFT, self.sp)
        cnt = torch.tensor([float(stack.oriFT.shape[0])], dtype=torch.float64, device=self.device)
        avg, ps, cnt = (_all_reduce(t, hemisphere_group) for t in (avg, ps, cnt))
        self.avg_sum, self.ps_sum = avg, ps
        self._set(*sigma_init_finalise(avg.cpu().numpy(), ps.cpu().numpy(), float(cnt[0]),
                                       self.idim, self.n_group, self.n_col))
        return self.sig, self.sig_rcp

    @staticmethod
    def alpha_of(stack):
        """sqrt(pi (maskRadius / (size pixelSize))^2), src/Optimiser.cpp:6686."""
        return math.sqrt(math.pi * (stack.r_mask / stack.N) ** 2)

    def update(self, stack, vol, rot, trans, pf=2, offS=None, dF=None, cls=None, group=None,
               alpha=None, hemisphere_group=None):
        """allReduceSigma: residual spectra at the given poses, per-group sums
        (group [n] int32 0-based; None = the ungrouped rule, row 0 for all),
        all-reduce, finalise.  Returns (sig, sigRcp)."""
        spectra, _ = residual_spectra(vol, stack.imgFT, stack.oriFT, stack.attr, rot, trans,
                                      self.sp, pf, offS, dF, cls)
        acc = sigma_accumulate(spectra, group, self.n_group)
        self.spectra = spectra
        self.acc = _all_reduce(acc, hemisphere_group)
        self._set(*sigma_finalise(self.acc, self.n_col,
                                  self.alpha_of(stack) if alpha is None else alpha,
                                  group is not None))
        return self.sig, self.sig_rcp

    def sig_rcp_rows(self, px, group=None, n=None):
        """allocPreCal's sigRcpP [n, nPxl] float32 on the device for pixel set
        px (ops.PixelSet): row group[l] (None: row 0, n images) at px.iSig.
        Expectation.run and the ops take it as it is; Stack.pixel_batch
        converts its sig_rcp through numpy, so hand it ``rows.cpu()``."""
        if self.sig_rcp_d is None:
            raise ValueError("no sigma yet: call init_from or update")
        if group is not None:
            n = group.shape[0]
            _req(group, torch.int32, (n,), "group")
        elif n is None:
            raise ValueError("sig_rcp_rows: give group or n")
        i_sig = torch.from_numpy(np.ascontiguousarray(px.iSig, np.int32)).to(self.device)
        out = torch.empty(n, px.n, dtype=torch.float32, device=self.device)
        for l0 in range(0, n, 65535):
            nb = min(65535, n - l0)
            check(lib().thx_sig_rcp_rows(_ptr(self.sig_rcp_d), self.n_group, self.n_col,
                                         _ptr(group[l0:]) if group is not None else None,
                                         _ptr(i_sig), px.n, nb, _ptr(out[l0:]),
                                         _stream(self.device)), "thx_sig_rcp_rows")
        return out

    def norms(self, stack, vol, rot, trans, r_l, r_norm, pf=2, dF=None, cls=None):
        """normCorrection's norm[l] = sum |img_l - CTF P(t)|^2, rL^2 <= i^2+j^2 <
        rNorm^2 (NORM_MASK: imgFT, t without the offset)."""
        return residual_spectra(vol, stack.imgFT, None, stack.attr, rot, trans, self.sp, pf, None,
                                dF, cls, norm_radii=(r_l, r_norm))[1]

    def norm_correction(self, stack, vol, rot, trans, r_l, r_norm, pf=2, dF=None, cls=None,
                        hemisphere_group=None):
        """normCorrection: norms, their median over all images of the group
        (gsl quantile at 0.5: the mean of the two middle values of an even
        count), stack.imgFT / oriFT scaled in place by sqrt(median / norm).
        Returns (norm [n] float64, median)."""
        norm = self.norms(stack, vol, rot, trans, r_l, r_norm, pf, dF, cls)
        every = norm
        if hemisphere_group is not None:
            import torch.distributed as dist
            parts = [None] * dist.get_world_size(hemisphere_group)
            dist.all_gather_object(parts, norm.cpu(), group=hemisphere_group)
            every = torch.cat(parts)
        m = float(np.median(every.cpu().numpy()))
        img_scale(stack.imgFT, stack.oriFT, torch.sqrt(m / norm).float())
        return norm, m
