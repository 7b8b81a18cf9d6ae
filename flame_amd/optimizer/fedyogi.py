"""FedYogi -- drop-in for lib/python/flame/optimizer/fedyogi.py:25-36."""
import torch

from .fedopt import FedOPT


class FedYogi(FedOPT):
    """FedYogi class: v = v - (1-beta_2)*d**2*sign(v - d**2) (fedyogi.py:34-36)."""

    variant = "fedyogi"

    def __init__(self, beta_1=0.9, beta_2=0.99, eta=1e-2, tau=1e-3, defer: bool = False, *,
                 clip_threshold=None, nonfinite: str = "keep", trim=None, krum=None,
                 krum_select=None, rfa=None, rfa_nu=None, noise_factor=None,
                 noise_seed=None):
        super().__init__(beta_1, beta_2, eta, tau, defer=defer, clip_threshold=clip_threshold, nonfinite=nonfinite,
                         trim=trim, krum=krum, krum_select=krum_select, rfa=rfa, rfa_nu=rfa_nu,
                         noise_factor=noise_factor, noise_seed=noise_seed)

    def _delta_v_tensor(self, v, d):
        return v - (1 - self.beta_2) * d**2 * torch.sign(v - d**2)
