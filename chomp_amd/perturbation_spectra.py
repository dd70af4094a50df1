"""perturbation_spectra.PerturbationTheory (perturbation_spectra.py:36-345) over the HIP library:
the F2 / F3 kernels, the tree-level bispectrum and the trispectrum run in k_pt
(csrc/chomp_pt_kernels.h), one configuration per lane, with the epoch's linear spectrum as
SingleEpoch.linear_power computes it.

The reference's methods keep their single-configuration meaning: the vector forms take length-3
arrays (the reference's numpy.vdot would flatten anything longer), the *_len, *_kdiff and
*_parallelogram forms scalars or broadcastable arrays.  bispectrum_many / trispectrum_many take
(N, 3) arrays, or contiguous float64 torch cuda tensors, and return one value per configuration.

Kept as shipped: set_redshift stores the redshift and then raises AttributeError (the
`set_redshif` typo, :85-87); a SingleEpoch passed at another redshift is moved there, which
mutates the caller's object (:70-71); Fs3 and Fs3_BCGS disagree (the trispectrum docstring says
"Failed tests - needs debugging").
"""
import numpy

from . import _lib
from . import cosmology


def alpha_BCGS(k1, k2):
    """Eq. 39 of BCGS (perturbation_spectra.py:36-44); 0 when k1 = 0."""
    k1sq = numpy.vdot(k1, k1)
    if k1sq == 0.0:
        return 0.0
    return numpy.vdot(k1 + k2, k1) / k1sq


def gamma_BCGS(k1, k2):
    """Eq. 68 of BCGS (perturbation_spectra.py:47-56); 0 when k1 or k2 = 0."""
    k1a = numpy.vdot(k1, k1)
    k2a = numpy.vdot(k2, k2)
    if k1a * k2a == 0.:
        return 0.0
    return 1 - (numpy.vdot(k1, k2)) ** 2 / (k1a * k2a)


def _vec(k):
    v = numpy.asarray(k, dtype=numpy.float64)
    if v.shape != (3,):
        raise ValueError("a wavevector is a length-3 array, got shape %r" % (v.shape,))
    return v


def _many(k):
    if _lib._is_torch(k):
        if k.dim() != 2 or k.shape[1] != 3:
            raise ValueError("wavevectors are an (N, 3) array, got shape %r" % (tuple(k.shape),))
        return k
    v = numpy.asarray(k, dtype=numpy.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("wavevectors are an (N, 3) array, got shape %r" % (v.shape,))
    return v


class PerturbationTheory(object):
    """Bispectrum and trispectrum from perturbation theory (perturbation_spectra.py:59-345)."""

    def __init__(self, redshift=0.0, cosmo_single_epoch=None, **kws):
        self._redshift = redshift
        if cosmo_single_epoch is None:
            cosmo_single_epoch = cosmology.SingleEpoch(redshift)
        elif cosmo_single_epoch._redshift != redshift:
            cosmo_single_epoch.set_redshift(redshift)     # mutates the caller's object (:70-71)
        self.cosmo = cosmo_single_epoch

    def set_cosmology(self, cosmo_dict, redshift=None):
        if redshift is None:
            redshift = self._redshift
        self.cosmo.set_cosmology(cosmo_dict, redshift)
        self._redshift = redshift

    def set_cosmology_object(self, cosmo_single_epoch):
        self.cosmo = cosmo_single_epoch
        self._redshift = self.cosmo._redshift

    def set_redshift(self, redshift):
        """:85-87 as shipped: the redshift is stored, then the misspelt call raises."""
        self._redshift = redshift
        raise AttributeError("'SingleEpoch' object has no attribute 'set_redshif'")

    # -- device ------------------------------------------------------------------
    def _eval(self, form, args):
        """The form on the configurations args [N, arity] for this object's epoch: [N]."""
        ctx = self.cosmo._dev()
        out = ctx.pt_eval(form, args, 0, 1)
        return out[0]

    def _vector_form(self, form, *ks):
        out = self._eval(form, numpy.concatenate([_vec(k) for k in ks]))
        return out[0]

    def _scalar_form(self, form, *cols):
        arrs = numpy.broadcast_arrays(*[numpy.asarray(c, dtype=numpy.float64) for c in cols])
        shape = arrs[0].shape
        out = self._eval(form, numpy.stack([a.ravel() for a in arrs], axis=1))
        return out.reshape(shape) if shape else out[0]

    def _many_form(self, form, *ks):
        ks = [_many(k) for k in ks]
        n = ks[0].shape[0]
        if any(k.shape[0] != n for k in ks):
            raise ValueError("every wavevector array needs the same number of rows")
        if _lib._is_torch(ks[0]):
            import torch
            args = torch.cat(ks, dim=1).contiguous()
            return self.cosmo._dev().pt_eval(form, args, 0, 1)[0]
        return self._eval(form, numpy.concatenate(ks, axis=1))

    # -- reference surface ---------------------------------------------------------
    def Fs2(self, k1, k2):
        """Eq. A.2 in GGRW (:89-105); 5/7 when |k1| or |k2| < 1e-8."""
        return self._vector_form("Fs2", k1, k2)

    def Fs2_len(self, k1, k2, z):
        """:107-123: lengths and the cosine z."""
        return self._scalar_form("Fs2_len", k1, k2, z)

    def Fs2_kdiff(self, k1, k2, mu):
        """:125-132: Fs2(k1 - k2, k2) from lengths (z divided by the squared length, as shipped)."""
        return self._scalar_form("Fs2_kdiff", k1, k2, mu)

    def Fs3(self, k1, k2, k3):
        """Eq. A.3 in GGRW (:147-180)."""
        return self._vector_form("Fs3", k1, k2, k3)

    def Fs3_parallelogram(self, k1, k2, mu):
        """:182-199: Fs3(k1, -k1, k2)."""
        return self._scalar_form("Fs3_parallelogram", k1, k2, mu)

    def F3(self, k1, k2, k3):
        """Eq. 73 in BCGS (:201-223)."""
        return self._vector_form("F3", k1, k2, k3)

    def Fs3_BCGS(self, k1, k2, k3, F3=None):
        """:225-229 with the default F3.  Another F3 is a Python callable: outside the
        accelerated scope (ChompScopeError)."""
        if F3 is not None and not (getattr(F3, "__self__", None) is self and
                                   getattr(F3, "__func__", None) is PerturbationTheory.F3):
            raise _lib.ChompScopeError(
                "Fs3_BCGS (perturbation_spectra.py:225-229) with a user F3 integrates a Python "
                "callable: outside the accelerated scope")
        return self._vector_form("Fs3_BCGS", k1, k2, k3)

    def bispectrum(self, k1, k2, k3):
        """Eq. 22 in CH (:231-249)."""
        return self._vector_form("bispectrum", k1, k2, k3)

    def bispectrum_len(self, k1, k2, k3, z12, z13, z23):
        """:251-259."""
        return self._scalar_form("bispectrum_len", k1, k2, k3, z12, z13, z23)

    def trispectrum(self, k1, k2, k3, k4):
        """Eq. 24 in CH (:261-310); NaN zeroed for p12 and p34 only."""
        return self._vector_form("trispectrum", k1, k2, k3, k4)

    def trispectrum_parallelogram(self, k1, k2, mu):
        """Eq. 7 in SZH (:312-345)."""
        return self._scalar_form("trispectrum_parallelogram", k1, k2, mu)

    # -- many configurations (no counterpart in the reference) -----------------------
    def bispectrum_many(self, k1, k2, k3):
        """bispectrum of N configurations: k1, k2, k3 (N, 3) arrays or torch cuda tensors."""
        return self._many_form("bispectrum", k1, k2, k3)

    def trispectrum_many(self, k1, k2, k3, k4):
        """trispectrum of N configurations: k1..k4 (N, 3) arrays or torch cuda tensors."""
        return self._many_form("trispectrum", k1, k2, k3, k4)
