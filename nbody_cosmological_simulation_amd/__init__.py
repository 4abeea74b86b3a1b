"""MI355X-native direct-summation N-body engine behind the reference's GalaxySimulation API.

Hot path: hand-written HIP kernels for gfx950 (csrc/) behind the C-ABI of include/nbody_amd.h,
called through ctypes (_native.py).  See DESIGN.md.
"""
from .quantization import (PrecisionMode, quantize_distance_squared, quantize_force, _grid_quantize,
                           _grid_quantize_safe, get_mode_from_string, describe_mode)
from .simulation import GalaxySimulation, run_comparison
from .ensemble import (GalaxyEnsemble, QuantizedEnsemble, EnergyHistory, EnsembleMetrics, check_record_arguments,
                       check_metrics_arguments, StabilityReport, check_member_ticks_arguments, explosion_reason,
                       CrashMeasures, CrashPointReport, crash_kind, crash_value, crash_severity, Divergence, DivergenceHistory,
                       check_mode_list, check_divergence_arguments, entropy_bits, divergence_rate, FineGridEnsemble,
                       check_fine_grid_arguments, RaggedEnsemble, check_ragged_arguments, RaggedQuantizedEnsemble,
                       check_ragged_grid_arguments)

__all__ = ["GalaxySimulation", "GalaxyEnsemble", "QuantizedEnsemble", "FineGridEnsemble", "check_fine_grid_arguments", "RaggedEnsemble", "check_ragged_arguments", "RaggedQuantizedEnsemble", "check_ragged_grid_arguments","EnergyHistory", "EnsembleMetrics", "check_record_arguments", "check_metrics_arguments", "StabilityReport", "check_member_ticks_arguments", "explosion_reason", "CrashMeasures", "CrashPointReport", "crash_kind", "crash_value", "crash_severity", "Divergence", "DivergenceHistory", "check_mode_list", "check_divergence_arguments", "entropy_bits", "divergence_rate", "run_comparison", "PrecisionMode", "quantize_distance_squared",
           "quantize_force", "_grid_quantize", "_grid_quantize_safe", "get_mode_from_string",
           "describe_mode"]
