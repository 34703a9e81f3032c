"""The fixed table of operators on spin bases WITHOUT permutation symmetries -- the whole 2^L space, one weight, and their sectors of
the global flip X alone -- that tests/test_gpu_unprojected_operators.py runs through every k_direct / packet / replicated-x path and
tests/test_unprojected_cases.py validates without a GPU.  The families are those of tests/projected_cases.py (all rings).  What each
row is there for:

  tfim, xyz, twist on 2^L     identity index (inversion: the identity index of L - 1 sites); xyz and twist have coefficients that
                              depend on the PARTNER's bits, twist is a real matrix with complex coefficients and is not Hermitian
  chiral, jq at one weight    combinadic index, three- and four-bit flip masks, complex coefficients (chiral)
  dimer_xxz, two_domain       exchange pairs of two amplitudes: pair kernels, sorted packet streams, the staged row kernel
  phase_hop, hop              directed runs of a complex / a real amplitude, not Hermitian
  *_36_3, *_40_3, *_34_3      64-bit words
"""
import functools

from projected_cases import make_config

# name -> (family, basis arguments of make_config, the MATRIX is real, it is Hermitian, number of basis states)
CASES = {
    "tfim_12": ("tfim", dict(L=12), True, True, 4096),
    "tfim_12_x-1": ("tfim", dict(L=12, X=-1), True, True, 2048),
    "xyz_12": ("xyz", dict(L=12), True, True, 4096),
    "xyz_12_x1": ("xyz", dict(L=12, X=1), True, True, 2048),
    "twist_12": ("twist", dict(L=12), True, False, 4096),
    "twist_13_x-1": ("twist", dict(L=13, X=-1), True, False, 4096),
    "chiral_12_full_x1": ("chiral", dict(L=12, X=1), False, True, 2048),
    "chiral_14_7": ("chiral", dict(L=14, weight=7), False, True, 3432),
    "chiral_14_7_x-1": ("chiral", dict(L=14, weight=7, X=-1), False, True, 1716),
    "jq_14_5": ("jq", dict(L=14, weight=5), True, True, 2002),
    "dimer_14_7": ("dimer_xxz", dict(L=14, weight=7), True, True, 3432),
    "two_domain_14_7_x1": ("two_domain", dict(L=14, weight=7, X=1), True, True, 1716),
    "phase_hop_14_7": ("phase_hop", dict(L=14, weight=7), False, False, 3432),
    "hop_14_7": ("hop", dict(L=14, weight=7), True, False, 3432),
    "chiral_36_3": ("chiral", dict(L=36, weight=3), False, True, 7140),
    "jq_40_3": ("jq", dict(L=40, weight=3), True, True, 9880),
    "phase_hop_34_3": ("phase_hop", dict(L=34, weight=3), False, False, 5984),
}
ALL = list(CASES)
HERMITIAN = [name for name, row in CASES.items() if row[3]]
NON_HERMITIAN = [name for name, row in CASES.items() if not row[3]]
INVERSION = [name for name, row in CASES.items() if "X" in row[1]]
FIXED_WEIGHT = [name for name, row in CASES.items() if "weight" in row[1]]


def config_of(name):
    family, args = CASES[name][:2]
    return make_config(family, **args)


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(basis states ascending, H on them as scipy.sparse.csr, leak) of a case, computed once per process"""
    from sector_reference import sector_matrix

    return sector_matrix(config_of(name))
