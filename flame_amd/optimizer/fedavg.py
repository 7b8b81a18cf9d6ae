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

One selection stage (``FedAvg._select``) stands between the cache and the reduction, for this class,
FedProx, FedGFT and the FedOPT family alike, and for every combination of the four opt-in kwargs
below.  It is a straight pipeline -- refuse, pop, measure, policy, select, rates:
what the round refuses is refused with the cache still full; the entries are popped in
``cache.iterkeys()`` order; the updates are measured at most once; the ``nonfinite`` policy and the
clip scales come from the sums of squares; krum selects among what is left, rfa weights it; rates and
scales are formed last.  With every kwarg at its default the stage is the reference's pop loop and nothing else.
What the kwargs refuse of each other, of ``defer=True`` and of the sharded wrapper is one table,
``flame_amd/optimizer/refusals.py``.

* Update guard (``clip_threshold=C``, ``nonfinite="skip"``; ``guard.py``): measured by
  ``engine.update_stats`` (each update's norm over the float tensors and its non-finite count); the
  rates come from what is left of ``total`` and the reduction takes the clip scales
  (``flame_agg_reduce_scaled``).  ``update_stats`` holds the round's records.
* Trimmed mean / median (``trim=2``, ``trim=0.1``, ``trim="median"``; ``trim.py``): the weighted
  average of the float keys is replaced by the coordinate-wise trimmed mean of what the stage left
  (``engine.trimmed_mean``, kernel ``flame_agg_trimmed``), added onto ``base_weights`` in place.
  ``trim_method="select"`` / ``"auto"`` lifts the chain kernel's ``k <= 16`` by the radix-selection
  kernel (``engine.selected_mean``, kernel ``flame_agg_select``).
* Krum / Multi-Krum (``krum=2``, ``krum=0.2``, ``krum_select=1``; ``krum.py``): measured by
  ``engine.update_gram`` (the pairwise Gram matrix, kernel ``flame_update_gram``) instead; its diagonal
  is the guard's sum of squares, so the guard costs no second pass.  Every update is scored on the
  host by its distances to its nearest neighbours and the selected ones are averaged with equal
  weights through the reduction above.
* Geometric median (``rfa=3``, ``rfa_nu=1e-6``; ``rfa.py``): measured by ``engine.update_stats``, whose
  sums of squares are the first squared distances (the centre starts at the unchanged model); each
  further Weiszfeld iteration is one reduction into a scratch centre and one ``engine.update_dist``
  (kernel ``flame_update_dist``).  Every eligible update is kept, with the final weights as its rate.

Behind the stage and the reduction, server-side Gaussian noise (``noise_factor=s``, ``noise_seed=``;
``noise.py``): one draw per round of standard deviation ``s * sqrt(fsum(rate^2))`` over the entries
actually aggregated (``engine.noise_fill``, kernel ``flame_noise_fill``), accumulated into the float
keys as one more update with rate 1 behind the last entry.  ``noise_round`` counts the noised rounds.
"""
import collections
import collections.abc
import copy
import logging
import math
import weakref

import torch

from .. import engine, metrics
from . import guard, refusals
from . import krum as krum_
from . import noise as noise_
from . import rfa as rfa_
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
            if dt in engine.MX_CODE:
                engine.mx_route(acc, [w], k, self._base[k].shape)        # an MX arrival: what the flush would refuse of it, now
            elif dt != acc:
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

    chain_defer = False        # FedOPT's deferred eager chain (an instance attribute there)

    def __init__(self, defer: bool = False, max_pending: int = 256, max_pending_bytes: int = 16 << 30, *,
                 clip_threshold=None, nonfinite: str = "keep", trim=None, krum=None, krum_select=None,
                 rfa=None, rfa_nu=None, noise_factor=None, noise_seed=None, trim_method=None):
        self.agg_weights = None
        self.regularizer = Regularizer()
        self.defer = defer
        self.max_pending = max_pending
        self.max_pending_bytes = max_pending_bytes
        self._deferred = None      # the DeferredWeights the last deferred do() returned
        self.clip_threshold, self.nonfinite = guard.check_kwargs(clip_threshold, nonfinite)
        self.trim = trim_.check_kwarg(trim)
        self.trim_method = trim_.check_method(trim_method, self.trim)
        self.krum, self.krum_select = krum_.check_kwargs(krum, krum_select)
        self.update_stats = []     # the last do()'s UpdateRecords, in cache order (empty: nothing measured)
        self.trim_k = None         # the last trimmed do()'s k
        self.trim_kernel = None    # ... and its kernel, "chain" or "select"
        self.krum_records = []     # the last krum do()'s KrumRecords, in cache order
        self.rfa, self.rfa_nu = rfa_.check_kwargs(rfa, rfa_nu)
        self.rfa_records = []      # the last rfa do()'s RfaRecords, in cache order
        self.rfa_trace = []        # ... and its (dist2, weights) per Weiszfeld iteration run, over the eligible updates
        self.noise_factor, self.noise_seed = noise_.check_kwargs(noise_factor, noise_seed)
        self.noise_round = 0       # the round counter fed to the generator: one per noised round
        self.noise_std = None      # the last noised round's standard deviation
        # every kwarg is valid: now what they refuse of each other and of a deferred queue (FedAvg's or FedOPT's)
        refusals.check(self, *[c for c in ("clip_threshold", "trim", "krum", "rfa") if refusals.is_set(self, c)],
                       *(("defer",) if defer or self.chain_defer else ()))

    @property
    def guarded(self) -> bool:
        return guard.is_set(self.clip_threshold, self.nonfinite)

    def _check_round(self, n, kwargs=()):
        """What a round of ``n`` updates refuses (stage step 1: before anything is popped): the sharded
        wrapper's key groups, and an ``n`` that krum or trim cannot take.  Returns krum's ``(f, q, m)``."""
        if "flame_amd_key_groups" in kwargs:
            refusals.check(self, "key_groups")
        if self.krum is not None:
            return krum_.check_round(self.krum, self.krum_select, n, engine.gram_max_clients())
        if self.trim is not None:
            self._trim_route(n)

    def _trim_route(self, n):
        """``(k, kernel)`` of a trimmed round of ``n`` updates, or its refusal (``trim.py``)."""
        if self.trim_method is None:
            return trim_.check_round(self.trim, n, engine.trimmed_max_k()), trim_.CHAIN
        return trim_.route(self.trim, self.trim_method, n, engine.trimmed_max_k, engine.select_max_clients)

    def _select(self, cache, total, kwargs=()):
        """THE selection stage of a round, for every class and every combination of the update guard,
        ``trim`` and ``krum``: refuse, pop, measure, policy, select, rates.  Returns
        ``(entries, scales)``: ``[(weights, rate)]`` in cache order -- empty when nothing is left to
        aggregate, as for an empty cache -- and the clip scales, None unless some update is clipped
        (the plain reduction then runs)."""
        if self.krum is None and self.trim is None and self.rfa is None and not self.guarded:
            # the plain round: after popping, the item is removed from the cache (fedavg.py:80-82);
            # rate = count / total; nothing is measured or recorded
            return [(tres.weights, tres.count / total) for tres in map(cache.pop, list(cache.iterkeys()))], None
        plan = self._check_round(len(cache), kwargs)                    # 1. refuse, the cache still full
        ends = list(cache.iterkeys())                                   # 2. pop, in cache.iterkeys() order
        popped = [cache.pop(e) for e in ends]
        n = len(ends)
        if self.krum is not None:                                       # 3. measure once
            gram, nonfinite = engine.update_gram([t.weights for t in popped])
            sumsq = gram.diagonal()                                     # the guard's sums of squares: no second pass
        elif self.guarded or self.rfa is not None:                      # (rfa: its first squared distances too)
            sumsq, nonfinite = engine.update_stats([t.weights for t in popped])
        kept, scales = list(range(n)), [1.0] * n
        if self.guarded:                                                # 4. the nonfinite policy and the clip scales
            refused = None
            try:
                records, kept, total = guard.apply_policy(ends, [t.count for t in popped], sumsq, nonfinite, total,
                                                          self.clip_threshold, self.nonfinite)
            except guard.NonFiniteUpdate as e:      # "raise": the records still say which ends were bad
                refused, records = e, e.records
            self.update_stats = records
            guard.save_metrics(self, records)
            if refused is not None:
                raise refused
            scales = [r.scale for r in records]
        if self.krum is not None:                                       # 5. select ...
            chosen, scores = [], [float("inf")] * n
            if kept:
                f, _, m = plan if len(kept) == n else self._check_round(len(kept))     # "skip" shrank the round
                scores_k, chosen_k = krum_.select(gram[kept][:, kept], nonfinite[kept], [scales[i] for i in kept], f, m)
                for pos, i in enumerate(kept):
                    scores[i] = scores_k[pos]
                chosen = [kept[pos] for pos in chosen_k]
            self.krum_records = krum_.records(ends, gram, nonfinite, scores, chosen)
            if kept:
                krum_.save_metrics(self, self.krum_records, f)
            rates = [1.0 / len(chosen) for _ in chosen]                 # 6. ... and rates: equal weights
        elif self.rfa is not None:                                      # 5. weigh: an update with a non-finite
            chosen = [i for i in kept if nonfinite[i] == 0 and math.isfinite(sumsq[i])]    # element is never read
            rates, dist2 = [], []
            if chosen:
                rates, dist2, self.rfa_trace = rfa_.iterate([popped[i].weights for i in chosen],
                                                            [sumsq[i] for i in chosen], self.rfa, self.rfa_nu)
            self.rfa_records = rfa_.records(ends, sumsq, nonfinite, chosen, dist2, rates)
            rfa_.save_metrics(self, self.rfa_trace)                     # 6. rates: the final Weiszfeld weights
        else:
            chosen = kept if total != 0 else []
            if chosen and len(chosen) != n:
                self._check_round(len(chosen))                          # trim: is what "skip" left enough?
            rates = [popped[i].count / total for i in chosen]           # 6. count / what is left of total
        scales = [scales[i] for i in chosen]
        return [(popped[i].weights, r) for i, r in zip(chosen, rates)], (scales if any(s != 1.0 for s in scales) else None)

    def do(self, base_weights, cache, *, total: int = 0, version: int = 0, **kwargs):
        """Aggregate the cached trainer updates into ``base_weights`` (in place)."""
        logger.debug("calling fedavg (flame_amd)")
        assert base_weights is not None
        self.update_stats = []     # this call's records only (an empty round measures nothing)
        self.krum_records = []
        self.rfa_records, self.rfa_trace = [], []
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
        if self.noise_factor is not None and "flame_amd_key_groups" in kwargs:
            refusals.check(self, "key_groups")      # the sharded wrapper, with the cache still full
        entries, scales = self._select(cache, total, kwargs)
        if not entries:                # nothing left to aggregate: as for an empty cache
            return None
        if self.trim is not None:
            # base_weights += the coordinate-wise trimmed mean of what the stage left (n of them)
            k, kernel = trim_.count(self.trim, len(entries)), trim_.CHAIN
            if self.trim_method is not None:
                k, kernel = self._trim_route(len(entries))
            mean = engine.selected_mean if kernel == trim_.SELECT else engine.trimmed_mean
            mean(base_weights, [w for w, _ in entries], k)
            self.trim_k, self.trim_kernel = k, kernel
            trim_.save_metrics(self, k, len(entries), kernel if self.trim_method is not None else None)
            return base_weights
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
        if self.noise_factor is not None:
            # one more update with rate 1 and scale 1 after the last entry, as a second reduction on the
            # same stream: the same bits as one launch over entries + [(noise, 1.0)], the slab fast path kept
            std, noise = self._draw_noise(self.agg_weights, entries)
            if noise:
                engine.accumulate(self.agg_weights, [(noise, 1.0)])
            self._noise_drawn(std)
        return self.agg_weights

    def _draw_noise(self, base_weights, entries, device=None):
        """This round's noise (the noise contract): ``std = s * sqrt(fsum(rate^2))`` over the
        entries actually aggregated, and ``{float key: round_dtype(z * std)}`` from ``engine.noise_fill`` for
        ``(noise_seed, noise_round)``."""
        std = noise_.std_of(self.noise_factor, [r for _, r in entries])
        return std, engine.noise_fill(base_weights, self.noise_seed, self.noise_round, std, device=device)

    def _noise_drawn(self, std):
        """A noised round has been issued: its metrics, and the counter moves on."""
        self.noise_std = std
        noise_.save_metrics(self, std, self.noise_round)
        self.noise_round += 1
