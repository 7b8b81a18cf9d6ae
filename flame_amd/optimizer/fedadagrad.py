"""FedAdaGrad -- drop-in for lib/python/flame/optimizer/fedadagrad.py:25-35."""
from .fedopt import FedOPT


class FedAdaGrad(FedOPT):
    """FedAdaGrad class: v = v + d**2 (fedadagrad.py:33-35)."""

    variant = "fedadagrad"

    def __init__(self, beta_1=0.9, beta_2=0.99, eta=1e-2, tau=1e-3, defer: bool = False, *,
                 clip_threshold=None, nonfinite: str = "keep", trim=None, krum=None,
                 krum_select=None, rfa=None, rfa_nu=None, noise_factor=None,
                 noise_seed=None):
        super().__init__(beta_1, beta_2, eta, tau, defer=defer, clip_threshold=clip_threshold, nonfinite=nonfinite,
                         trim=trim, krum=krum, krum_select=krum_select, rfa=rfa, rfa_nu=rfa_nu,
                         noise_factor=noise_factor, noise_seed=noise_seed)

    def _delta_v_tensor(self, v, d):
        return v + d**2
