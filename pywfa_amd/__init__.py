"""pywfa_amd — MI355X-native batched wavefront aligner behind pywfa's interface.

Same names as ``pywfa/__init__.py`` of the reference, plus ``AlignmentResult``, ``left_align_ops`` and ``QualitySet`` (the handle
``WavefrontAligner.quality_set`` returns).
"""
from .align import (WavefrontAligner, AlignmentResult, QualitySet, clip_cigartuples, cigartuples_to_str,  # noqa: F401
                    elide_mismatches_from_cigar, left_align_ops)

__all__ = ["WavefrontAligner", "AlignmentResult", "QualitySet", "clip_cigartuples", "cigartuples_to_str",
           "elide_mismatches_from_cigar", "left_align_ops"]
__version__ = "0.1.0"
