"""The ``trim`` kwarg: coordinate-wise trimmed-mean / median aggregation in place of the weighted
average (Yin et al., ICML 2018, "Byzantine-Robust Distributed Learning: Towards Optimal
Statistical Rates"; flame has no counterpart -- its ``OptimizerType`` is a closed enum, so the
reachable form is a kwarg of the existing classes, like the update guard's).

The update guard bounds an update's *norm*.  An update that is wrong coordinate by coordinate
with a plausible norm (label-flipped trainers, a stuck sensor, a replayed stale model, a
sign-flipped delta scaled to the median norm) passes it; the trimmed mean drops, per element, the
``k`` smallest and the ``k`` largest of the ``n`` values before averaging the rest.

``trim`` is ``None`` (the default: nothing here runs), an int ``k >= 0``, a float fraction in
``[0, 0.5)`` (``k = floor(trim * n)``, the floor of the Python float product) or ``"median"``
(``k = (n - 1) // 2``: one value kept for odd ``n``, the mean of two for even ``n``).  ``n`` is
the number of updates aggregated by that ``do()``.  ``count`` and ``total`` play no part in the
float keys: a weighted trimmed mean would let a liar choose its own weight.  Integer / bool keys
are averaged with equal weights ``1 / n`` by the existing statement; no robustness is claimed for
counters.  The arithmetic is stated in DESIGN.md §2 and ``include/flame_amd.h``.
"""
import math

from .. import metrics

MEDIAN = "median"


def check_kwarg(trim):
    """Validate the constructor kwarg; returns it (a float fraction as float, an int as int)."""
    if trim is None:
        return None
    if isinstance(trim, bool):
        raise TypeError("trim must be None, an int >= 0, a float in [0, 0.5) or 'median', not a bool")
    if isinstance(trim, str):
        if trim != MEDIAN:
            raise ValueError(f"trim must be 'median' when a string, not {trim!r}")
        return trim
    if isinstance(trim, int):
        if trim < 0:
            raise ValueError(f"trim must be >= 0, not {trim!r}")
        return trim
    if isinstance(trim, float):
        if not (0.0 <= trim < 0.5):          # a NaN fails both
            raise ValueError(f"trim as a fraction must lie in [0, 0.5), not {trim!r}")
        return trim
    raise TypeError(f"trim must be None, an int >= 0, a float in [0, 0.5) or 'median', not {type(trim).__name__}")


def count(trim, n: int) -> int:
    """The trim count ``k`` of a round of ``n`` updates."""
    if trim == MEDIAN:
        return max(0, (n - 1) // 2)
    if isinstance(trim, float):
        return int(math.floor(trim * n))
    return int(trim)


def check_round(trim, n: int, max_k: int) -> int:
    """``k`` for ``n`` updates, or the round's refusal: ValueError when ``n <= 2k`` (nothing
    would be kept), NotImplementedError when ``k`` exceeds the kernels' chain capacity."""
    k = count(trim, n)
    if n <= 2 * k:
        raise ValueError(f"flame_amd trim={trim!r}: k = {k} needs more than {2 * k} updates, the round has {n}")
    if k > max_k:
        raise NotImplementedError(
            f"flame_amd trim={trim!r}: k = {k} for {n} updates exceeds the selection kernels' capacity of {max_k} "
            f"(the median exists for n <= {2 * max_k + 2}); a selection for larger k is a follow-up (DESIGN.md §8)")
    return k


def save_metrics(owner, k: int, n: int) -> None:
    """``trim_k`` / ``updates_trimmed_from`` beside the kernel metrics."""
    mc, alias = metrics.collector(owner)
    if mc is None:
        return
    mc.save("trim_k", alias, k)
    mc.save("updates_trimmed_from", alias, n)
