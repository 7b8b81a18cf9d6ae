"""FedAvg on MI355X -- drop-in for lib/python/flame/optimizer/fedavg.py:30-104.

Same contract as the reference: ``base_weights`` is mutated in place and
returned (fedavg.py:74,87); cache entries are consumed with ``cache.pop`` in
``cache.iterkeys()`` order (:79-82); ``rate = count / total`` (:84); ``None``
when the cache is empty or ``total == 0`` (:76-77); extra kwargs such as
``num_trainers`` are accepted and ignored.

The reference's O(N x #tensors) Python loop of two torch ops
(``_aggregate_pytorch``, :89-104) becomes one HIP launch per dtype
(``flame_agg_reduce``) over every key and every client, with the per-element
client order kept sequential so results are bit-identical.

Eager batching (opt-in, ``FedAvg(defer=True)``, e.g. the job config's optimizer
``kwargs``): the eager top aggregator calls ``do()`` once per arrival on the same
``base_weights`` with the running total (``eager_syncfl/top_aggregator.py:36-90``), which
as written reads and writes the whole model per arrival (3 passes of P per update).
Each arrival's rate ``count / total`` is fixed when it arrives, so with ``defer=True``
``do()`` queues it and returns a :class:`DeferredWeights` -- a read-only Mapping over
``base_weights`` -- and the queued arrivals are reduced into ``base_weights`` in ONE
launch, with the identical per-element operation sequence (bit-identical), the moment
anything reads the result (``w[k]``, ``items()``, ``load_state_dict``, ``deepcopy``), a
``do()`` arrives with another base dict, an empty ``do()`` returns ``None``, or
``max_pending`` arrivals / ``max_pending_bytes`` are queued.  ``base_weights`` itself
(a plain dict) lags until then: read the returned object, as flame's roles do.

Server-side update guard (opt-in, ``FedAvg(clip_threshold=C, nonfinite="skip")``, see
``flame_amd/optimizer/guard.py``): ``do()`` measures every popped update once
(``engine.update_stats``: its norm over the float tensors and its non-finite count), applies
the ``nonfinite`` policy, forms the rates from the remaining ``total`` and reduces with the
clip scales (``flame_agg_reduce_scaled``).  ``update_stats`` holds the round's records.
With both kwargs at their defaults none of this runs.

Trimmed mean / median (opt-in, ``FedAvg(trim=2)``, ``trim=0.1``, ``trim="median"``, see
``flame_amd/optimizer/trim.py``): ``do()`` replaces the weighted average of the float keys by the
coordinate-wise trimmed mean of the popped updates (``engine.trimmed_mean``, kernel
``flame_agg_trimmed``), added onto ``base_weights`` in place.  The ``nonfinite`` policies run
first.  ``trim`` with ``clip_threshold``, ``defer=True`` or the sharded wrapper is refused.  With
``trim=None`` (the default) none of this runs.

Krum / Multi-Krum (opt-in, ``FedAvg(krum=2)``, ``krum=0.2``, ``krum_select=1``, see
``flame_amd/optimizer/krum.py``): ``do()`` measures the round's pairwise Gram matrix once
(``engine.update_gram``, kernel ``flame_update_gram``), scores every update by its distances to its
nearest neighbours on the host, and averages the selected ones with equal weights through the
reduction above.  The Gram's diagonal is the guard's sum of squares, so ``clip_threshold`` and
``nonfinite`` cost no second measuring pass.  ``krum`` with ``trim``, ``defer=True`` or the sharded
wrapper is refused.  With ``krum=None`` (the default) none of this runs.
"""
import collections
import collections.abc
import copy
import logging
import weakref

import torch

from .. import engine, metrics
from . import guard
from . import krum as krum_
from . import trim as trim_
from .abstract import AbstractOptimizer
from .fedbuff import _own_shm_views
from .regularizer import Regularizer

logger = logging.getLogger(__name__)


class DeferredWeights(collections.abc.Mapping):
    """``base_weights`` plus queued eager arrivals, reduced into it on first read."""

    def __init__(self, base, max_pending, max_pending_bytes=None, owner=None):
        self._base = base
        # the optimizer (weakly: it holds this object; a cycle would keep queued slab slots
        # alive until the cyclic GC): its metric_collector sees the flush's launch
        self._owner = weakref.ref(owner) if owner is not None else None
        self._pending = []         # [(weights, rate)] in arrival order
        self._max_pending = max_pending
        self._max_bytes = max_pending_bytes
        self._held = 0             # bytes of queued arrivals that own their memory (not slab slots)
        self._arrival_bytes = sum(v.numel() * v.element_size() for v in base.values()
                                  if isinstance(v, torch.Tensor))

    def _check(self, w):
        # the reference raises from the do() that brought a bad arrival (fedavg.py:93-104):
        # unknown keys, and `agg += tmp` whose promoted dtype cannot be cast back to the aggregate's
        for k in w.keys():
            if k not in self._base:
                raise KeyError(k)
            acc, dt = self._base[k].dtype, engine.weight_dtype(w, k)
            if dt != acc:
                engine._check_cast(acc, dt)

    def _queue(self, entries):
        for w, _ in entries:
            self._check(w)
        # a view into a sender's shared-memory segment is copied to HBM before do() returns
        entries = [(_own_shm_views(w), r) for w, r in entries]
        self._pending.extend(entries)
        self._held += sum(self._arrival_bytes for w, _ in entries if getattr(w, "slab", None) is None)
        if len(self._pending) >= self._max_pending or (self._max_bytes is not None and self._held > self._max_bytes):
            self.flush()

    @property
    def pending(self):
        return len(self._pending)

    def flush(self):
        """Reduce every queued arrival into ``base_weights`` (one launch per dtype)."""
        if not self._pending:
            return
        entries, self._pending, self._held = self._pending, [], 0
        with metrics.recording(self._owner() if self._owner is not None else None):
            engine.accumulate(self._base, entries)

    def __getitem__(self, k):
        self.flush()
        return self._base[k]

    def __iter__(self):
        return iter(self._base)

    def __len__(self):
        return len(self._base)

    def __contains__(self, k):
        return k in self._base

    def __deepcopy__(self, memo):
        self.flush()
        return copy.deepcopy(self._base, memo)

    def __reduce__(self):
        # pickling (torch.save, a checkpoint) stores the reduced model as a state_dict-style OrderedDict
        return (collections.OrderedDict, (list(self.items()),))

    def materialize(self):
        """``base_weights`` itself, every queued arrival reduced into it."""
        self.flush()
        return self._base


class FedAvg(AbstractOptimizer):
    """FedAvg class."""

    def __init__(self, defer: bool = False, max_pending: int = 256, max_pending_bytes: int = 16 << 30, *,
                 clip_threshold=None, nonfinite: str = "keep", trim=None, krum=None, krum_select=None):
        self.agg_weights = None
        self.regularizer = Regularizer()
        self.defer = defer
        self.max_pending = max_pending
        self.max_pending_bytes = max_pending_bytes
        self._deferred = None      # the DeferredWeights the last deferred do() returned
        self._init_guard(clip_threshold, nonfinite, defer)
        self._init_trim(trim, defer)
        self._init_krum(krum, krum_select, defer)

    def _init_krum(self, krum, krum_select, defer):
        self.krum, self.krum_select = krum_.check_kwargs(krum, krum_select)
        self.krum_records = []     # the last krum do()'s KrumRecords, in cache order
        if self.krum is None:
            return
        if getattr(self, "trim", None) is not None:
            krum_.refuse(f"{type(self).__name__}(trim=...)", self.krum,
                         "two robust rules in one round have no stated meaning; choose trim or krum")
        if defer or getattr(self, "chain_defer", False):
            krum_.refuse(f"{type(self).__name__}(defer=True)", self.krum,
                         "Krum scores every update against the round's others; use defer=False")

    def _init_trim(self, trim, defer):
        self.trim = trim_.check_kwarg(trim)
        self.trim_k = None         # the last trimmed do()'s k
        if self.trim is None:
            return
        if self.clip_threshold is not None:
            trim_.refuse(f"{type(self).__name__}(clip_threshold=...)", self.trim,
                         "a clipped update would be trimmed on its scaled values, which needs the scale inside "
                         "the selection kernel (a follow-up); use nonfinite= alone with trim")
        if defer or getattr(self, "chain_defer", False):
            trim_.refuse(f"{type(self).__name__}(defer=True)", self.trim,
                         "a trimmed mean needs every update of the round at once; use defer=False")

    def _init_guard(self, clip_threshold, nonfinite, defer):
        self.clip_threshold, self.nonfinite = guard.check_kwargs(clip_threshold, nonfinite)
        self.update_stats = []     # the last do()'s UpdateRecords, in cache order (empty: nothing measured)
        if defer or getattr(self, "chain_defer", False):     # FedAvg's queue or FedOPT's chain
            guard.refuse(f"{type(self).__name__}(defer=True)", self.clip_threshold, self.nonfinite,
                         "a deferred queue fixes each arrival's rate when it arrives, before the guard "
                         "could measure it; use defer=False")

    @property
    def guarded(self) -> bool:
        return guard.is_set(self.clip_threshold, self.nonfinite)

    def _pop_entries(self, cache, total):
        # after popping, the item is removed from the cache (fedavg.py:80-82); rate = count / total
        return [(tres.weights, tres.count / total) for tres in map(cache.pop, list(cache.iterkeys()))]

    def _pop_guarded(self, cache, total):
        """_pop_entries under the update guard: pop, measure every update once, apply the
        ``nonfinite`` policy, and only then form the rates from what is left of ``total``.
        Returns ``(entries, scales)``; ``entries`` is empty when every update was skipped,
        ``scales`` None when no update is clipped (the plain reduction then runs)."""
        ends = list(cache.iterkeys())
        popped = [cache.pop(e) for e in ends]
        sumsq, nonfinite = engine.update_stats([t.weights for t in popped])
        try:
            records, kept, total = guard.apply_policy(ends, [t.count for t in popped], sumsq, nonfinite, total,
                                                      self.clip_threshold, self.nonfinite)
        except guard.NonFiniteUpdate as e:      # "raise": the records still say which ends were bad
            self.update_stats = e.records
            guard.save_metrics(self, e.records)
            raise
        self.update_stats = records
        guard.save_metrics(self, records)
        if not kept or total == 0:
            return [], None
        entries = [(popped[i].weights, popped[i].count / total) for i in kept]
        scales = [records[i].scale for i in kept]
        return entries, (scales if any(s != 1.0 for s in scales) else None)

    def _check_krum(self, cache, kwargs):
        """What a krum round refuses before anything is popped; returns ``(f, q, m)``."""
        if "flame_amd_key_groups" in kwargs:
            krum_.refuse("ShardedOptimizer", self.krum,
                         "each rank holds a slice of every update; its partial Gram matrices would need an "
                         "all-reduce before the selection (a follow-up)")
        return krum_.check_round(self.krum, self.krum_select, len(cache), engine.gram_max_clients())

    def _pop_krum(self, cache, total, kwargs):
        """_pop_guarded's sibling under ``krum``: pop, measure the round's Gram matrix once, let the
        guard (if set) decide on its diagonal and the non-finite counts, select, and give the
        selected updates the rate ``1 / len(selected)``.  Returns ``(entries, scales)`` as
        _pop_guarded does; ``entries`` is empty when nothing can be selected."""
        f, q, m = self._check_krum(cache, kwargs)
        ends = list(cache.iterkeys())
        popped = [cache.pop(e) for e in ends]
        gram, nonfinite = engine.update_gram([t.weights for t in popped])
        kept = list(range(len(ends)))
        scales = [1.0] * len(ends)
        if self.guarded:
            try:
                records, kept, _ = guard.apply_policy(ends, [t.count for t in popped], gram.diagonal(), nonfinite,
                                                      total, self.clip_threshold, self.nonfinite)
            except guard.NonFiniteUpdate as e:      # "raise": the records still say which ends were bad
                self.update_stats = e.records
                guard.save_metrics(self, e.records)
                raise
            self.update_stats = records
            guard.save_metrics(self, records)
            scales = [r.scale for r in records]
            if len(kept) != len(ends):          # "skip" shrank the round
                if not kept:
                    self.krum_records = krum_.records(ends, gram, nonfinite, [float("inf")] * len(ends), [])
                    return [], None
                f, q, m = krum_.check_round(self.krum, self.krum_select, len(kept), engine.gram_max_clients())
        idx = list(kept)
        scores_k, selected_k = krum_.select(gram[idx][:, idx], nonfinite[idx], [scales[i] for i in idx], f, m)
        scores = [float("inf")] * len(ends)
        for pos, i in enumerate(idx):
            scores[i] = scores_k[pos]
        selected = [idx[pos] for pos in selected_k]
        self.krum_records = krum_.records(ends, gram, nonfinite, scores, selected)
        krum_.save_metrics(self, self.krum_records, f)
        if not selected:
            return [], None
        entries = [(popped[i].weights, 1.0 / len(selected)) for i in selected]
        sel_scales = [scales[i] for i in selected]
        return entries, (sel_scales if any(s != 1.0 for s in sel_scales) else None)

    def _do_trimmed(self, base_weights, cache, total, kwargs):
        """do() under ``trim``: base_weights += the coordinate-wise trimmed mean of the cached
        updates.  A round that cannot be trimmed (``n <= 2k``, or ``k`` beyond the kernels'
        capacity) raises before anything is popped.  Under a ``nonfinite`` policy the updates are
        popped and measured first, as the guard does, and ``n`` is what remains."""
        if "flame_amd_key_groups" in kwargs:
            trim_.refuse("ShardedOptimizer", self.trim,
                         "each rank would trim its own slices in waves; the selection kernel takes no key groups "
                         "yet (a follow-up)")
        max_k = engine.trimmed_max_k()
        k = trim_.check_round(self.trim, len(cache), max_k)
        if self.guarded:
            entries, _ = self._pop_guarded(cache, total)
            if not entries:            # every update skipped: as for an empty cache
                return None
            if len(entries) != len(self.update_stats):
                k = trim_.check_round(self.trim, len(entries), max_k)
        else:
            entries = self._pop_entries(cache, total)
        engine.trimmed_mean(base_weights, [w for w, _ in entries], k)
        self.trim_k = k
        trim_.save_metrics(self, k, len(entries))
        return base_weights

    def do(self, base_weights, cache, *, total: int = 0, version: int = 0, **kwargs):
        """Aggregate the cached trainer updates into ``base_weights`` (in place)."""
        logger.debug("calling fedavg (flame_amd)")
        assert base_weights is not None
        self.update_stats = []     # this call's records only (an empty round measures nothing)
        self.krum_records = []
        if isinstance(base_weights, DeferredWeights):
            base_weights = base_weights.materialize()
        pend = self._deferred
        if pend is not None and (pend._base is not base_weights or len(cache) == 0 or total == 0
                                 or not self.defer or "flame_amd_key_groups" in kwargs):
            # another base dict, an empty round or a non-deferred call: the queued arrivals
            # land in their base dict first, as the reference's in-place adds would have
            pend.flush()
            self._deferred = pend = None
        self.agg_weights = base_weights
        if len(cache) == 0 or total == 0:
            return None
        if self.trim is not None:
            return self._do_trimmed(base_weights, cache, total, kwargs)
        scales = None
        if self.krum is not None:
            entries, scales = self._pop_krum(cache, total, kwargs)
            if not entries:            # nothing eligible: as for an empty cache
                return None
        elif self.guarded:
            entries, scales = self._pop_guarded(cache, total)
            if not entries:            # every update skipped: as for an empty cache
                return None
        else:
            entries = self._pop_entries(cache, total)
        if self.defer and "flame_amd_key_groups" not in kwargs:
            if pend is None:
                self._deferred = pend = DeferredWeights(base_weights, self.max_pending, self.max_pending_bytes,
                                                        owner=self)
            pend._queue(entries)
            return pend
        # flame_amd.shard passes its plan's waves: one launch per wave, its all-gather started
        # right behind it (callers from flame pass no such kwargs)
        extra = {} if scales is None else {"scales": scales}     # only a clipped round names them
        engine.accumulate(self.agg_weights, entries, key_groups=kwargs.get("flame_amd_key_groups"),
                          after_group=kwargs.get("flame_amd_after_group"), **extra)
        return self.agg_weights
