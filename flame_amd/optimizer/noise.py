"""Server-side Gaussian noise: the second half of flame's differential-privacy statement, on the aggregator.

flame's trainer clips its delta to ``clip_threshold`` (``privacy/differential_privacy.py:63-84``) and
then adds ``torch.normal(0, noise_factor)`` to every element (``:55-61``).  The update guard restates
the clip on the aggregator (``guard.py``); this module restates the noise there (DP-FedAvg, McMahan
et al., ICLR 2018).  ``noise_factor`` has the name and meaning of the job's
``privacy.kwargs.noise_factor``: the standard deviation of the noise *per update*.  n independent
per-trainer draws of variance ``s^2`` give the weighted average ``sum(rate_i * update_i)`` a variance of
``s^2 * sum(rate_i^2)``; the aggregator draws that distribution once:

    std   = s * sqrt(fsum(rate_i^2))          in Python floats, over the entries actually aggregated
    noise = round_dtype(z * std)              engine.noise_fill: Philox4x32-10 + Box-Muller, float keys only
    out   = round(acc + round(noise * 1))     one more update with rate 1 and scale 1, after the last entry

``noise_seed`` (an int in ``[0, 2^64)``; ``None`` draws 8 bytes from ``os.urandom`` at construction) and
the round counter ``noise_round`` make every draw reproducible.  This is the reference's fp32
``torch.normal`` statement moved to the server, not a hardened DP sampler; accounting (epsilon, delta)
is the operator's.
"""
import math
import os

from .. import metrics


def check_kwargs(noise_factor, noise_seed):
    """Validate the two constructor kwargs; returns ``(noise_factor as float or None, noise_seed as int or
    None)``.  ``noise_factor=0`` is ``None``; the seed is only drawn or checked when the factor is set."""
    if noise_factor is not None:
        if isinstance(noise_factor, bool) or not isinstance(noise_factor, (int, float)):
            raise TypeError(f"noise_factor must be a number or None, not {type(noise_factor).__name__}")
        noise_factor = float(noise_factor)
        if not (noise_factor >= 0.0) or math.isinf(noise_factor):
            raise ValueError(f"noise_factor must be a finite number >= 0, not {noise_factor!r}")
        if noise_factor == 0.0:
            noise_factor = None
    if noise_seed is not None:
        if isinstance(noise_seed, bool) or not isinstance(noise_seed, int):
            raise TypeError(f"noise_seed must be an int or None, not {type(noise_seed).__name__}")
        if not 0 <= noise_seed < 1 << 64:
            raise ValueError(f"noise_seed must lie in [0, 2^64), not {noise_seed!r}")
    elif noise_factor is not None:
        noise_seed = int.from_bytes(os.urandom(8), "little")
    return noise_factor, noise_seed


def std_of(noise_factor: float, rates) -> float:
    """``s * sqrt(fsum(rate_i^2))`` in Python floats: the standard deviation the reference's n
    per-trainer draws of ``noise_factor`` give the weighted average with these rates."""
    return float(noise_factor) * math.sqrt(math.fsum(float(r) * float(r) for r in rates))


def save_metrics(owner, std: float, rnd: int) -> None:
    """``noise_std`` / ``noise_round`` beside the kernel metrics."""
    mc, alias = metrics.collector(owner)
    if mc is None:
        return
    mc.save("noise_std", alias, std)
    mc.save("noise_round", alias, rnd)
