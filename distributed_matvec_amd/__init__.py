"""Import alias: the package directory is ``distributed-matvec_amd/`` (not a valid Python
identifier), so ``import distributed_matvec_amd`` resolves its submodules from there."""
import os as _os

__path__.insert(0, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "..", "distributed-matvec_amd"))

from .api import *  # noqa: F401,F403,E402
from . import api as _api  # noqa: E402
from .entanglement import *  # noqa: F401,F403,E402
from . import entanglement as _entanglement  # noqa: E402
from . import correlations  # noqa: E402  (the module keeps its name here too: its driver is correlations.correlations)
from .correlations import (CorrelationPlan, FermionCorrelations, SpinCorrelations, fermion_correlations, spin_correlations,  # noqa: F401,E402
                           structure_factor)
from . import expectation  # noqa: E402  (the module keeps its name here: its driver is expectation.expectation)
from .expectation import (ExpectationPlan, dimer_correlations, eigenstate_matrix_elements, expectation_values,  # noqa: F401,E402
                          expectation_values_block, matrix_elements, pair_correlations)
from . import evolve  # noqa: E402  (the module keeps its name here: its driver is evolve.evolve)
from .evolve import (EvolveResult, ThermalCorrelationResult, ThermalExpectationResult, autocorrelation, bessel_series,  # noqa: F401,E402
                     combine_sector_expectations, combine_sectors, propagate, propagator_coefficients, thermal_correlation,
                     thermal_expectation)
from . import projection  # noqa: E402
from .projection import SectorProjection, product_state, project  # noqa: F401,E402
from . import sampling  # noqa: E402
from .sampling import SectorAmplitudes, amplitudes, sample_states, snapshots  # noqa: F401,E402
from . import kpm  # noqa: E402
from .kpm import (KpmMatrixResult, block_gram, chebyshev_moment_matrices, cross_correlation, greens_matrix,  # noqa: F401,E402
                  moment_matrices_from_grams, reconstruct_matrix, spectral_matrix)

_kpm_matrix = ["KpmMatrixResult", "block_gram", "chebyshev_moment_matrices", "cross_correlation", "greens_matrix",
               "moment_matrices_from_grams", "reconstruct_matrix", "spectral_matrix"]
__all__ = _kpm_matrix + list(_api.__all__) + list(_entanglement.__all__) + list(projection.__all__) + list(sampling.__all__) + [n for n in correlations.__all__ if n != "correlations"] + [n for n in expectation.__all__ if n != "expectation"] + [n for n in evolve.__all__ if n != "evolve"]
