"""FedAdam -- drop-in for lib/python/flame/optimizer/fedadam.py:25-35."""
from .fedopt import FedOPT


class FedAdam(FedOPT):
    """FedAdam class: v = beta_2*v + (1-beta_2)*d**2 (fedadam.py:33-35)."""

    variant = "fedadam"

    def __init__(self, beta_1=0.9, beta_2=0.99, eta=1e-2, tau=1e-3, defer: bool = False, *,
                 clip_threshold=None, nonfinite: str = "keep", trim=None, krum=None,
                 krum_select=None, rfa=None, rfa_nu=None, noise_factor=None,
                 noise_seed=None):
        super().__init__(beta_1, beta_2, eta, tau, defer=defer, clip_threshold=clip_threshold, nonfinite=nonfinite,
                         trim=trim, krum=krum, krum_select=krum_select, rfa=rfa, rfa_nu=rfa_nu,
                         noise_factor=noise_factor, noise_seed=noise_seed)

    def _delta_v_tensor(self, v, d):
        return self.beta_2 * v + (1 - self.beta_2) * d**2
