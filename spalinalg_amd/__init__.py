"""spalinalg_amd -- MI355X (gfx950) SpMV / assembly path for spalinalg.

Host-side mirror of the reference's public types (`CsrMatrix`, `CscMatrix`,
`CooMatrix`; reference src/lib.rs:16-19) over the C ABI of libspal_hip.so
(include/spal.h).  The compute path is hand-written HIP only; there is no
CPU fallback.
"""
from ._ffi import Panic, SpalError, cache_trim, device_count  # noqa: F401
from .matrix import (Amg, Fsai, fsai_row, CooMatrix, CscMatrix, CsrMatrix, DeviceCoo, DeviceCsr, DeviceCsc, EigshInfo, KpmInfo, KrylovInfo, MultiGpuCsr,  # noqa: F401
                     amg_aggregate, cheb_delta_coefficients, dot, dot_dev, kpm_count, kpm_damping, kpm_density, kpm_probes)

__all__ = ["CsrMatrix", "CscMatrix", "CooMatrix", "DeviceCsr", "DeviceCsc", "DeviceCoo", "MultiGpuCsr", "Panic",
           "SpalError", "device_count", "cache_trim", "dot", "dot_dev", "KrylovInfo", "EigshInfo", "Amg",
           "amg_aggregate", "Fsai", "fsai_row", "cheb_delta_coefficients", "KpmInfo", "kpm_probes", "kpm_damping", "kpm_density", "kpm_count"]
