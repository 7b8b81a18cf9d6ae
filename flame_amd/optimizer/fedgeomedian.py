"""FedGeoMedian -- ``FedAvg(rfa=...)`` under a name of its own, for direct use (flame's
``OptimizerType`` is a closed enum, so it is not registered as a drop-in; a job reaches the same
code through its optimizer ``kwargs``, see ``flame_amd/optimizer/rfa.py``).
"""
from .fedavg import FedAvg


class FedGeoMedian(FedAvg):
    """The geometric median of the round's updates (RFA, Pillutla et al. 2022): ``iters`` smoothed
    Weiszfeld iterations with the smoothing floor ``nu``."""

    def __init__(self, iters=5, nu=1e-6, *, nonfinite: str = "keep"):
        if iters is None:
            raise TypeError("FedGeoMedian needs iters (an int >= 1)")
        super().__init__(nonfinite=nonfinite, rfa=iters, rfa_nu=nu)
