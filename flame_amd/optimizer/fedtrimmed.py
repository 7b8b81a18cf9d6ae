"""FedTrimmedMean / FedMedian -- ``FedAvg(trim=...)`` under names of their own, for direct use
(flame's ``OptimizerType`` is a closed enum, so they are not registered as drop-ins; a job
reaches the same code through its optimizer ``kwargs``, see ``flame_amd/optimizer/trim.py``).
"""
from . import trim as trim_
from .fedavg import FedAvg


class FedTrimmedMean(FedAvg):
    """Coordinate-wise trimmed mean: ``trim`` an int ``k``, a fraction in [0, 0.5) or ``"median"``;
    ``trim_method`` None (the chain kernel, ``k <= 16``), ``"select"`` or ``"auto"`` (any ``k``)."""

    def __init__(self, trim, *, nonfinite: str = "keep", trim_method=None):
        if trim is None:
            raise TypeError("FedTrimmedMean needs a trim (an int >= 0, a float in [0, 0.5) or 'median')")
        super().__init__(nonfinite=nonfinite, trim=trim, trim_method=trim_method)


class FedMedian(FedTrimmedMean):
    """Coordinate-wise median (``k = (n - 1) // 2``).  With ``trim_method`` left at None the chain
    kernel's capacity bounds the round at 2 * max_k + 2 = 34 updates; ``trim_method="select"`` or
    ``"auto"`` takes rounds of up to ``engine.select_max_clients()`` updates (65,535) on the
    radix-selection kernel."""

    def __init__(self, *, nonfinite: str = "keep", trim_method=None):
        super().__init__(trim_.MEDIAN, nonfinite=nonfinite, trim_method=trim_method)
