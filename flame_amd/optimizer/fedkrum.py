"""FedMultiKrum / FedKrum -- ``FedAvg(krum=...)`` under names of their own, for direct use
(flame's ``OptimizerType`` is a closed enum, so they are not registered as drop-ins; a job
reaches the same code through its optimizer ``kwargs``, see ``flame_amd/optimizer/krum.py``).
"""
from .fedavg import FedAvg


class FedMultiKrum(FedAvg):
    """Multi-Krum: ``f`` assumed bad updates (an int, or a fraction in [0, 0.5)); the ``select``
    lowest scores are averaged (default ``n - f``)."""

    def __init__(self, f, *, select=None, clip_threshold=None, nonfinite: str = "keep"):
        if f is None:
            raise TypeError("FedMultiKrum needs f (an int >= 0 or a float in [0, 0.5))")
        super().__init__(clip_threshold=clip_threshold, nonfinite=nonfinite, krum=f, krum_select=select)


class FedKrum(FedMultiKrum):
    """Krum: the single update with the lowest score becomes the round's average."""

    def __init__(self, f, *, clip_threshold=None, nonfinite: str = "keep"):
        super().__init__(f, select=1, clip_threshold=clip_threshold, nonfinite=nonfinite)
