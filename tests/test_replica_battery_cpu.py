"""Keeps the battery of the replica tests (tests/replica_util.py) complete as the ABI grows, and
checks its starts where no device is needed.

Every output entry point of include/nghmm.h has a twin nghmm_chain_<name> over a chain of site
shards, declared there or in another public header under include/ (nghmm_chain_long.h); the command line runs all of them on a replica whenever replicate 1 does not win a
multi-start run.  So every single-handle function with such a twin must be in replica_util.COVERED,
and the battery must really call what COVERED names."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import replica_util as ru
import support_util as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# read-back entry points without a chain twin that every run's output files go through
ALSO = {"nghmm_viterbi", "nghmm_get_posteriors", "nghmm_get_gl", "nghmm_geno_posteriors",
        "nghmm_format_posteriors", "nghmm_lkl_batch"}


def _public_headers():
    """Every header under include/ but the debugging one: nghmm.h and what declares a twin apart
    from it (nghmm_chain_long.h)."""
    return sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h") and f != "nghmm_debug.h")


def _declared(*headers):
    headers = headers or _public_headers()
    text = "".join(open(os.path.join(ROOT, "include", f)).read() for f in headers)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"\b(nghmm_[a-z_0-9]+)\s*\(", text))


def test_every_output_entry_point_is_in_the_battery():
    names = _declared()
    twins = {n for n in names if not n.startswith("nghmm_chain_") and "nghmm_chain_" + n[len("nghmm_"):] in names}
    # (the rule finds the output entry points: the list is checked so that a change of naming
    # cannot empty it unnoticed)
    assert {"nghmm_ibd_tracts", "nghmm_sample_paths", "nghmm_tract_support", "nghmm_tract_bounds",
            "nghmm_freq_info", "nghmm_geno_smooth", "nghmm_obs_info", "nghmm_ibd_summary",
            "nghmm_ibd_expect", "nghmm_ibd_moments", "nghmm_ibd_by_length", "nghmm_ibd_longest",
            "nghmm_ibd_long", "nghmm_ibd_sharing"} <= twins
    assert ALSO <= names
    missing = sorted((twins | ALSO) - ru.COVERED)
    assert not missing, f"entry points without a replica test (tests/replica_util.py): {missing}"
    # (nghmm_get_emissions, the e_prob read-back, is declared next to the debugging entry points)
    unknown = sorted(ru.COVERED - names - _declared("nghmm_debug.h"))
    assert not unknown, f"COVERED names what the headers do not declare: {unknown}"


def test_the_battery_calls_what_covered_names(pkg):
    """The C functions behind the NgsFHMM methods and properties that battery() uses on its
    handle are exactly a superset of COVERED."""
    hm = importlib.import_module("ngsf-hmm_amd.hmm")
    used = set(re.findall(r"\bh\.([A-Za-z_][A-Za-z_0-9]*)", inspect.getsource(ru.battery)))
    used |= {"_get"} if used & {"indF", "alpha", "freq"} else set()
    reached = set()
    for attr in used:
        member = inspect.getattr_static(hm.NgsFHMM, attr, None)
        fn = member.fget if isinstance(member, property) else member
        if fn is not None and callable(fn):
            reached |= set(re.findall(r"self\.lib\.(nghmm_[a-z_0-9]+)", inspect.getsource(fn)))
    missing = sorted(ru.COVERED - reached)
    assert not missing, f"COVERED names entry points that battery() does not call: {missing}"


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_the_starts_differ_in_every_key_the_oracle_has(pkg, orc_det, packed):
    """The non-vacuity condition of tests/test_gpu_replica_outputs.py, on the oracle for the keys it
    has: one EM iteration and a decode from each of the battery's starts on the 20 x 5003 cohort
    give different indF, alpha, freq, ind_lkl, posteriors, paths, emissions and .geno posteriors,
    for every pair of starts."""
    import orclib
    cohort = sup.gpu_cohort(pkg)
    d, gl = cohort[0], cohort[1]
    if packed:
        gl = orc_det.prepare_gl(d.gl, 0, call_geno=True)
    res = []
    for start in ru.starts(d.n_ind, d.n_sites, 2):
        em = orclib.OracleEM(orc_det, gl, d.pos_dist_mb)
        em.set_params(*start)
        assert em.init_emission() == 0 and em.iterate() == 0
        path = em.viterbi()
        res.append({"indF": em.indF, "alpha": em.alpha, "freq": em.freq, "ind_lkl": em.ind_lkl,
                    "marg_prob": em.marg, "path": path, "e_prob": em.e_prob,
                    "geno_posteriors": em.geno_post(path)})
        em.close()
    a, b = res
    for k in a:
        assert a[k].tobytes() != b[k].tobytes(), k
    # ... and clearly, not by a last bit: whole tracts are decoded differently
    cells = np.mean(a["path"] != b["path"])
    print(f"paths differ at {cells:.3f} of the cells, largest |d posterior| "
          f"{np.abs(a['marg_prob'] - b['marg_prob']).max():.3f}")
    assert cells > 0.01
