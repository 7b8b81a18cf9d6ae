"""FedTrimmedMean / FedMedian -- ``FedAvg(trim=...)`` under names of their own, for direct use
(flame's ``OptimizerType`` is a closed enum, so they are not registered as drop-ins; a job
reaches the same code through its optimizer ``kwargs``, see ``flame_amd/optimizer/trim.py``).
"""
from . import trim as trim_
from .fedavg import FedAvg


class FedTrimmedMean(FedAvg):
    """Coordinate-wise trimmed mean: ``trim`` an int ``k``, a fraction in [0, 0.5) or ``"median"``."""

    def __init__(self, trim, *, nonfinite: str = "keep"):
        if trim is None:
            raise TypeError("FedTrimmedMean needs a trim (an int >= 0, a float in [0, 0.5) or 'median')")
        super().__init__(nonfinite=nonfinite, trim=trim)


class FedMedian(FedTrimmedMean):
    """Coordinate-wise median (``k = (n - 1) // 2``; n <= 2 * max_k + 2 = 34 updates per round)."""

    def __init__(self, *, nonfinite: str = "keep"):
        super().__init__(trim_.MEDIAN, nonfinite=nonfinite)
