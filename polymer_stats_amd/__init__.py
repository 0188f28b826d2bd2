"""polymer_stats_amd -- MI355X (gfx950) implementation of the fixed-force-ensemble MCMC hot path of
grasingerm/polymer-stats (mcmc_eap_chain.jl), behind the C ABI of include/pstat.h.

_lib, ensemble: the binding.  free_energy: A(r) from recorded histograms (numpy only).  mcmc_eap_chain, mcmc_clustering_eap_chain, mcmc_clustering_eap_chain_2d: the drop-in hosts of the
reference's three mains (python -m polymer_stats_amd.<name>), short modules over _host, which holds what they share.  sweep,
aggregate_mcmc: the reference's run/*.jl sweeps and scripts/aggregate_mcmc.jl.  julia_fmt: Julia's number formatting."""
from ._lib import (DIELECTRIC, POLAR, NONINTERACTING, INTERACTING, ISING, CUTOFF, F32, F64, Q16, RNG_MWC64X, RNG_XOSHIRO128PP, NOBS, NRED, NQ, MOVES_SINGLE, MOVES_CLUSTER,
                   OBS_NAMES, PLANAR_OBS_NAMES, PLANAR_OBS_INDEX, EB_NAMES, HC_NAMES, CORR_NAMES, SHAPE_NAMES, PDIST_NAMES, ENERGY_NAMES, HistSpec, hist_spec, Params, PstatError, default_params, default_planar_params)
from .ensemble import (Corr, CorrResult, Energy, EnergyResult, Ensemble, ErrorBars, Hist, HistResult, Pdist, PdistResult, Shape, ShapeResult, Tempering, blocking_device, histogram_device, ladders_by,
                       shape_anisotropy, summary_from_reduction)
from .free_energy import extension_free_energy, wham_force

__all__ = ["DIELECTRIC", "POLAR", "NONINTERACTING", "INTERACTING", "ISING", "CUTOFF", "F32", "F64", "Q16", "RNG_MWC64X", "RNG_XOSHIRO128PP", "NOBS",
           "NRED", "NQ", "MOVES_SINGLE", "MOVES_CLUSTER", "OBS_NAMES", "PLANAR_OBS_NAMES", "PLANAR_OBS_INDEX", "EB_NAMES", "Params", "PstatError",
           "default_params", "default_planar_params", "Ensemble", "ErrorBars", "Tempering", "blocking_device", "ladders_by",
           "summary_from_reduction", "HC_NAMES", "HistSpec", "hist_spec", "Hist", "HistResult", "histogram_device",
           "extension_free_energy", "wham_force", "CORR_NAMES", "Corr", "CorrResult",
           "SHAPE_NAMES", "Shape", "ShapeResult", "shape_anisotropy",
           "PDIST_NAMES", "Pdist", "PdistResult",
           "ENERGY_NAMES", "Energy", "EnergyResult"]
