"""Host helpers of the detection census (``GossipSim.detect_census``, ``gs_detect_census``): the ground-truth
clock the census measures detection latency against, the derived rates, and the threshold sweep.

The census compares the failure detector's live / dead sets (``FailureDetector.live_nodes`` / ``dead_nodes``,
``failure_detector.py:60-67``) and its phi values (``failure_detector.py:69-87``) with what the caller knows to
be true: which nodes are up, and since when the others have been down.

Beside ``DownClock`` and ``roc``: ``detect_rates`` (the three derived figures ``detect_census`` adds to its result)
and ``hist_quantile_bucket`` / ``max_bucket`` (the bucket summaries ``tools/detection.py`` prints).
"""

from __future__ import annotations

import numpy as np


class DownClock:
    """``down_since`` of a cluster of ``n`` nodes: the tick at which each down node went down.

    ``update(up, tick)`` records ``tick`` for every node that was up at the previous update and is down now; the
    first update treats a down node as going down at ``tick``.  Entries of up nodes keep their last value (the
    census ignores them)."""

    def __init__(self, n: int):
        self.n = int(n)
        self.down_since = np.zeros(self.n, dtype=np.uint32)
        self._was_up = np.ones(self.n, dtype=bool)

    def update(self, up, tick: int) -> np.ndarray:
        up = np.asarray(up.cpu() if hasattr(up, "cpu") else up).astype(bool)
        if up.shape != (self.n,):
            raise ValueError(f"up mask of {up.shape} for {self.n} nodes")
        self.down_since[self._was_up & ~up] = np.uint32(tick)
        self._was_up = up.copy()
        return self.down_since


def detect_rates(census: dict) -> dict:
    """The three derived figures of a census (denominators at least 1)."""
    return {
        "false_suspicion_rate": census["up_dead"] / max(1, census["up_pairs"]),
        "detected_fraction": census["down_dead"] / max(1, census["down_pairs"]),
        "undetected": census["down_live"],
    }


def merge_censuses(parts: list[dict]) -> dict:
    """Censuses of disjoint observer sets of one cluster (``GossipSim.detect_census_zoned``: one per component) as
    one: what ``gs_detect_census`` defines for slices, but over rows -- sums add, ``observers`` among them, maxima
    take the largest, the per-target counts add, the smallest time of death is the smallest and the largest the
    largest (-1 = nobody), the per-row counts add (a row is counted in one part).  ``ShardGroup.detect_census``
    merges over target columns instead (``observers`` taken once, per-target tensors joined), and all-reduces: the
    two do not share code."""
    from ._lib import DETECT_HIST_FIELDS, DETECT_MAX_FIELDS, DETECT_OVER_FIELDS, DETECT_TOTAL_FIELDS

    if not parts:
        raise ValueError("no census to merge")
    out = {k: (max if k in DETECT_MAX_FIELDS else sum)(p[k] for p in parts) for k in DETECT_TOTAL_FIELDS}
    for k in DETECT_HIST_FIELDS + DETECT_OVER_FIELDS:
        out[k] = [sum(p[k][b] for p in parts) for b in range(len(parts[0][k]))]
    out.update(detect_rates(out))
    for k in ("target_live_by", "target_dead_by", "row_false_suspicions", "row_undetected"):
        if k in parts[0]:
            acc = parts[0][k].clone()
            for p in parts[1:]:
                acc += p[k]
            out[k] = acc
    if "target_first_tod" in parts[0]:
        first, last = parts[0]["target_first_tod"].clone(), parts[0]["target_last_tod"].clone()
        for p in parts[1:]:
            f = p["target_first_tod"]
            both = (first >= 0) & (f >= 0)
            first = first.where(~both, first.minimum(f)).where(both | (first >= 0), f)
            last = last.maximum(p["target_last_tod"])
        out["target_first_tod"], out["target_last_tod"] = first, last
    return out


def roc(census: dict, thresholds) -> list[tuple[float, float, float]]:
    """``(threshold, up_over / up_phi, down_over / down_phi)`` per swept threshold: the share of the up targets'
    windows a detector with that ``phi_threshold`` would suspect (false suspicions) against the share of the down
    targets' windows it would (detections), over the pairs that have a phi."""
    thresholds = [float(x) for x in thresholds]
    if len(census["up_over"]) != len(thresholds) or len(census["down_over"]) != len(thresholds):
        raise ValueError("the census was not taken with these thresholds")
    return [(t, census["up_over"][i] / max(1, census["up_phi"]), census["down_over"][i] / max(1, census["down_phi"]))
            for i, t in enumerate(thresholds)]


def hist_quantile_bucket(hist, q: float = 0.5) -> int:
    """The bucket holding the ``q`` quantile of a census histogram (-1 when it is empty)."""
    total = sum(hist)
    if not total:
        return -1
    acc = 0
    for b, c in enumerate(hist):
        acc += c
        if acc >= q * total:
            return b
    return len(hist) - 1


def max_bucket(hist) -> int:
    """The highest non-empty bucket (-1 when the histogram is empty)."""
    nz = [b for b, c in enumerate(hist) if c]
    return nz[-1] if nz else -1
