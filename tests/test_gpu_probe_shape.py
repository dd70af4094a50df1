"""The shape of the mass-limit probes of a small batch (pytest -m gpu): chi(z) integrated beside
the sigma tables (k_sigma_nodes' chi rows) and the probes as one launch of wider blocks.  The
shape may move the last bits of a probe's nu, which nothing reads; it must not move a DECISION
(the step each mass-limit walk stops at, the count of its exact integrals) or chi.

tests/golden/probe_shape_parent.json holds this project's own output (hex floats) from before
the change of shape: ln M_min, ln M_max, n_search (the evaluations of both sides), chi and the
status word of
  wmap7_three            WMAP7 at z = 0, 0.75, 1.5 in one context,
  w0wa_middle            the same with w0 = -0.9, wa = 0.1 in the middle epoch,
  batch130_first_three   the first three epochs of a 130-epoch batch (the two-launch shape)."""
import json
import os

import numpy
import pytest

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

Z3 = [0.0, 0.75, 1.5]
K8 = numpy.logspace(-3, 2, 8)
FIELDS = ("ln_mass_min", "ln_mass_max", "chi")


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "probe_shape_parent.json")) as f:
        return json.load(f)


def _record(hg, n):
    """What the fixture holds, of the first n epochs of a set-up grid."""
    st = hg.status()
    out = []
    for i in range(n):
        sc = hg.ctx.scalars(i)
        out.append({"ln_mass_min": float(sc["ln_mass_min"]), "ln_mass_max": float(sc["ln_mass_max"]),
                    "n_search": int(sc["n_search"]), "chi": float(sc["chi"]), "status": int(st[i])})
    return out


def _same_as_parent(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert g[f] == float.fromhex(w[f]), (i, f, g[f].hex(), w[f])
        assert g["n_search"] == w["n_search"], (i, g["n_search"], w["n_search"])
        assert g["status"] == w["status"], (i, g["status"], w["status"])


@pytest.fixture(scope="module")
def three():
    from chomp_amd import grid
    hg = grid.HaloGrid(numpy.array(Z3))
    hg.setup("power_mm")
    return hg


@pytest.fixture(scope="module")
def oracle_epochs():
    from oracle import chomp_oracle as o
    return [o.epoch(None, z) for z in Z3]


def test_three_epochs_decide_as_before(three, parent, oracle_epochs):
    """1: the limits and the evaluation counts bit for bit; the nu table and P_mm against the
    oracle at test_gpu_halo's tolerances (nu 1e-7, P 1e-4)."""
    from oracle import chomp_oracle as o
    _same_as_parent(_record(three, 3), parent["wmap7_three"])
    got = three.power("power_mm", K8)
    for i, e in enumerate(oracle_epochs):
        m = o.mass_table(e)
        assert three.ctx.scalars(i)["ln_mass_min"] == m.ln_mass_min
        assert three.ctx.scalars(i)["ln_mass_max"] == m.ln_mass_max
        assert rel_err(three.ctx.table("nu", i), m.nu_arr) < 1e-7, i
        t = o.halo_table(e, m, families=("mm",))
        assert rel_err(got[i], o.halo_power(t, "mm", K8)) < 1e-4, i


def test_chi_beside_the_sigma_tables(three, parent, oracle_epochs):
    """2: chi bit-equal to the fixture and within 1e-13 of the oracle's."""
    for i, e in enumerate(oracle_epochs):
        chi = float(three.ctx.scalars(i)["chi"])
        assert chi == float.fromhex(parent["wmap7_three"][i]["chi"]), (i, chi.hex())
        assert abs(chi - e.chi) <= 1e-13 * abs(e.chi), (i, chi, e.chi)


def test_one_epoch_alone_equals_the_batch(three):
    """3: an epoch's chi and limits do not depend on its neighbours in the launch."""
    from chomp_amd import grid
    batch = _record(three, 3)
    for i, z in enumerate(Z3):
        hg = grid.HaloGrid(numpy.array([z]))
        hg.setup("power_mm")
        assert _record(hg, 1)[0] == batch[i], (i, z)


def test_fixed_mass_limits_still_get_chi(parent):
    """4: mass_min, mass_max > 0 skip the search (mass_function.py:163-170): the one working
    block of an epoch takes chi from its slot and writes the logarithms of the limits."""
    from chomp_amd import defaults, grid
    saved = dict(defaults.default_limits)
    try:
        defaults.default_limits.update(mass_min=1e10, mass_max=3e15)
        hg = grid.HaloGrid(numpy.array(Z3))
        hg.setup("power_mm")
        got = _record(hg, 3)
    finally:
        defaults.default_limits.clear()
        defaults.default_limits.update(saved)
    for i, g in enumerate(got):
        assert g["chi"] == float.fromhex(parent["wmap7_three"][i]["chi"]), (i, g["chi"].hex())
        assert g["ln_mass_min"] == numpy.log(1e10) and g["ln_mass_max"] == numpy.log(3e15), (i, g)
        assert g["n_search"] == 0 and g["status"] == 0, (i, g)


def test_dark_energy_chi_is_still_overwritten(parent):
    """5: a w0-wa epoch between two LCDM ones: its chi (k_de_chi, behind the probes) and
    everything else as before."""
    from chomp_amd import defaults, grid
    base = dict(defaults.default_cosmo_dict)
    hg = grid.HaloGrid(numpy.array(Z3), cosmo_dict=[dict(base), dict(base, w0=-0.9, wa=0.1), dict(base)])
    hg.setup("power_mm")
    got = _record(hg, 3)
    _same_as_parent(got, parent["w0wa_middle"])
    assert got[1]["chi"] != float.fromhex(parent["wmap7_three"][1]["chi"])


def test_large_batch_shape_is_untouched(parent):
    """6: 130 epochs take the two-launch shape, which shares constants with the small one."""
    from chomp_amd import grid
    hg = grid.HaloGrid(numpy.concatenate([Z3, numpy.linspace(0.01, 1.49, 127)]))
    hg.setup("power_mm")
    _same_as_parent(_record(hg, 3), parent["batch130_first_three"])
