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

``trim_method`` chooses the kernel of a trimmed round.  ``None`` (the default) is the chain kernel
alone (``engine.trimmed_mean``, ``k <= 16``; a larger ``k`` is refused).  ``"select"`` runs every
trimmed round on the radix-selection kernel (``engine.selected_mean``): any ``k`` with ``n > 2k``,
``n`` up to ``engine.select_max_clients()``.  ``"auto"`` takes the chain wherever it exists
(``k <= engine.trimmed_max_k()``) and the selection beyond.  Both kernels keep the same multiset
``sorted(x)[k : n - k]`` but add it in different orders (the chain in the order the values emerge,
the selection the inside values in client order and the ties at both ends last), so a chain round
and a select round of the same inputs can differ in the last bit; in practice that shows on f64
keys only, where the fp64 sum is itself rounded.
"""
import math

from .. import metrics

MEDIAN = "median"
SELECT, AUTO = "select", "auto"
CHAIN = "chain"             # the kernels' names in ``opt.trim_kernel`` and the ``trim_kernel`` metric: CHAIN / SELECT


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


def check_method(trim_method, trim):
    """Validate the ``trim_method`` kwarg beside an already validated ``trim``; returns it."""
    if trim_method is None:
        return None
    if not isinstance(trim_method, str):
        raise TypeError(f"trim_method must be None, 'select' or 'auto', not {type(trim_method).__name__}")
    if trim_method not in (SELECT, AUTO):
        raise ValueError(f"trim_method must be None, 'select' or 'auto', not {trim_method!r}")
    if trim is None:
        raise ValueError(f"trim_method={trim_method!r} needs a trim (it chooses the kernel of a trimmed round)")
    return trim_method


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


def route(trim, trim_method, n: int, max_k, max_clients):
    """``(k, kernel)`` for ``n`` updates under a ``trim_method`` that is set, or the round's refusal:
    ValueError when ``n <= 2k``, NotImplementedError when ``n`` exceeds the selection kernel's
    capacity.  ``max_k`` / ``max_clients`` are the engine's getters, called only where the answer
    depends on them."""
    k = count(trim, n)
    if n <= 2 * k:
        raise ValueError(f"flame_amd trim={trim!r}: k = {k} needs more than {2 * k} updates, the round has {n}")
    if trim_method == AUTO and k <= max_k():
        return k, CHAIN
    cap = max_clients()
    if n > cap:
        raise NotImplementedError(
            f"flame_amd trim={trim!r}, trim_method={trim_method!r}: {n} updates exceed the selection kernel's "
            f"capacity of {cap} (engine.select_max_clients)")
    return k, SELECT


def save_metrics(owner, k: int, n: int, kernel=None) -> None:
    """``trim_k`` / ``updates_trimmed_from`` beside the kernel metrics; ``trim_kernel`` under a ``trim_method``."""
    mc, alias = metrics.collector(owner)
    if mc is None:
        return
    mc.save("trim_k", alias, k)
    mc.save("updates_trimmed_from", alias, n)
    if kernel is not None:
        mc.save("trim_kernel", alias, kernel)
