"""What the wide 16-bit scan covers (include/mmf_hg_wide.h): ``ops.simtopk(..., precision="fast" | "fast_bf16")``
for feature dims above 1024, where the register-resident scan stops.  Host-only queries: no GPU is touched.
"""
from __future__ import annotations

from . import _lib


def wide_scan_supported(d: int, k: int, exclude_self: bool = True) -> bool:
    """True when ``ops.simtopk`` serves ``precision="fast"`` / ``"fast_bf16"`` at feature dim ``d`` through the wide scan:
    1024 < d <= 4096 and k + self <= 20 (d <= 1024 is ``ops.fast_scan_supported``'s)."""
    return bool(_lib.lib().mmf_wide_scan_supported(int(d), int(k), int(bool(exclude_self))))


def list_capacity(k: int, exclude_self: bool = True) -> int:
    """Entries of one candidate list of the wide scan (0: k + self beyond 20).  A row with at most this many columns inside
    its error-margin band is never sent to the exact rescan."""
    return int(_lib.lib().mmf_wide_scan_list_capacity(int(k), int(bool(exclude_self))))
