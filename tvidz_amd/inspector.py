"""Analysis driver + HTTP/SSE surface — restatement of /root/reference/inspector/app.py around the
GPU kernels (the reference's own loop cannot be kept: its scene scorer is a child process).

Kept from the reference, citation by citation:
  * key/filename hygiene and the unique analysis key            app.py:122-136
  * result record {status, scene_cuts, progress, total_cuts, duplicates, original_filename,
    clean_filename[, error]}                                    app.py:153-161, 294-302, 307-315
  * consecutive-duplicate drop of cut timestamps                app.py:231
  * persist the growing prefix, match with min_match=2, drop self, stop at the FIRST hit,
    store duplicate ids, report duplicate filenames             app.py:234-255
  * routes: POST /notify, GET /status/<f>, GET+OPTIONS /status/stream/<f> (SSE, emit on change,
    0.2 s tick, stop at done/error), /build-info, /admin/clear-db, /debug/*   app.py:23-115, 324-415
  * CORS headers on every response                              app.py:15-21

Changed on purpose (documented in DESIGN.md): frames are scored in micro-batches on the GPU and
every batch issues ONE match whose `kth` output reproduces the per-prefix loop; `progress` is
true frame progress when the frame count is known (the reference's `n:` parse never succeeds,
SURVEY.md §3.3); uploads run on a bounded worker pool instead of one unbounded thread each; the
SQS poller (app.py:417-480) is out of scope (no compute).

Per micro-batch the driver thread does: one H2D copy (copy stream), three kernel launches
(SAD, finalize, tail: the scene state stays on the device), ONE small device-to-host copy of the
compacted cut list + one event wait, and - only when the batch produced new cuts - one
find_duplicates (one launch + one stream sync) and one stream-ordered corpus upsert.  Staging
memory is a bounded pool shared by all uploads (feeder.SlotPool), sized in bytes, so 64 concurrent
4K uploads use the same ~2 GiB of pinned memory as 16 uploads of 480p (BASELINE configs[4]).
"""
from __future__ import annotations

import json
import os
import sys
import threading
import time
import uuid
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import scene
from .feeder import FrameFeeder, SlotPool, open_reader

KTH_NEVER = 0x7FFFFFFF


def split_filenames(key: str):
    """app.py:122-130: last path component, and the name without the `<digits>-` upload prefix."""
    filename = key.split("/")[-1] if key and "/" in key else key or "unknown_file"
    if not filename:
        filename = "unknown_file"
    original_filename = filename
    if "-" in filename and filename.split("-")[0].isdigit():
        original_filename = "-".join(filename.split("-")[1:])
    return filename, original_filename


def s3_frame_source(bucket: str, key: str, filename: str, unique_id: str):
    """app.py:163-200: fetch the object from LocalStack with 5 retries, then open a decoder."""
    import requests
    s3_url = f"http://localstack:4566/{bucket}/{key}"
    local_path = f"/tmp/{unique_id}_{filename}"
    last = None
    for attempt in range(5):
        try:
            r = requests.get(s3_url, stream=True)
            with open(local_path, "wb") as f:
                for chunk in r.iter_content(chunk_size=1 << 20):
                    f.write(chunk)
            if not os.path.exists(local_path) or not local_path.startswith("/tmp/"):
                raise Exception(f"Invalid or unsafe file path: {local_path}")
            return open_reader(local_path), local_path
        except Exception as e:
            last = e
            if attempt < 4:
                time.sleep(1)
    raise Exception(f"File download incomplete or corrupt after 5 attempts: {last}")


def _corpus_can(corpus, method: str, flag: str) -> bool:
    """Can the store's corpus answer `method`?  It has the method and, where it says so with a `flag` (a
    service.RankCorpus always has the method; whether its matcher has the form is its supports_* view), the flag is
    true - so what cannot be answered is refused when the driver is built, not inside an upload."""
    return hasattr(corpus, method) and bool(getattr(corpus, flag, True))


class Inspector:
    def __init__(self, store, device: str = "cuda:0", frame_source: Optional[Callable] = None,
                 threshold: float = scene.DEFAULT_THRESHOLD, min_match: int = 2,
                 pts_policy: str = scene.PTS_POLICY_G6, batch: int = 256, max_workers: int = 16,
                 near_duplicates: bool = False, near_eps: float = 1.0 / 30, near_max_offset: float = 30.0,
                 near_jaccard: float = 0.8, slot_bytes: int = 64 << 20, n_slots: Optional[int] = None,
                 profile: bool = False, match_tolerance: float = 0.0, near_top_k: Optional[int] = None,
                 near_any_offset: bool = False, near_score: str = "jaccard", near_min_votes: int = 1,
                 near_rates=None, near_spans: bool = False, near_parts: Optional[int] = None,
                 near_two_bins: bool = False, near_candidates: Optional[int] = None, near_gap_eps: float = 1.0 / 30,
                 near_candidate_rates: bool = False, near_parts_two_bins: bool = False,
                 near_candidates_long: bool = False):
        self.store = store
        # opt-in: the near-duplicate report from the K best-aligned rows the device keeps (tvz_align_topk) instead of
        # one row per corpus row walked here.  None: the walk, exactly as before.  Refused here where the store's
        # corpus cannot do it.
        self.near_top_k = None if near_top_k is None else int(near_top_k)
        if self.near_top_k is not None:
            if not 1 <= self.near_top_k <= 64:
                raise ValueError(f"near_top_k must be None or 1..64, got {near_top_k!r}")
            if not hasattr(getattr(store, "corpus", None), "align_topk"):
                raise RuntimeError(f"near_top_k={self.near_top_k}: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_topk; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus")
        # opt-in: the near-duplicate search at ANY shift (tvz_align_wide_topk, 2^22 bins of near_eps on either side
        # instead of near_max_offset) - the copy with its intro cut off, the excerpt, the compilation - and, with
        # near_score="containment", scored by v / min(n, row_len) so that the excerpt of a long video is not thrown
        # away by its Jaccard; near_min_votes keeps a row of one or two cuts from counting as contained by chance.
        # Defaults: the bounded search and the Jaccard, exactly as before.
        self.near_any_offset = bool(near_any_offset)
        self.near_score, self.near_min_votes = near_score, int(near_min_votes)
        if near_score not in ("jaccard", "containment", "local"):
            raise ValueError(f"near_score must be 'jaccard', 'containment' or 'local', got {near_score!r}")
        if self.near_min_votes < 1:
            raise ValueError(f"near_min_votes must be >= 1, got {near_min_votes!r}")
        if near_score == "containment" and not self.near_any_offset:
            raise ValueError("near_score='containment' needs near_any_offset=True (the score of tvz_align_wide_topk)")
        if self.near_any_offset:
            if not near_duplicates or self.near_top_k is None:
                raise ValueError("near_any_offset=True needs near_duplicates=True and near_top_k")
            if not _corpus_can(getattr(store, "corpus", None), "align_wide_topk", "supports_align_wide"):
                raise RuntimeError(f"near_any_offset=True: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_wide_topk; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus")
        # opt-in: the search at any shift for copies played at another speed (tvz_align_rates_topk) - every row is
        # aligned at each of near_rates (1..8 finite rates > 0, in the order of preference: stored ~= rate x upload +
        # shift) and reported once, at its best rate, with a "rate" field.  None: nothing changes.
        self.near_rates = None if near_rates is None else tuple(float(r) for r in near_rates)
        if self.near_rates is not None:
            if not 1 <= len(self.near_rates) <= 8 or not all(0.0 < r <= sys.float_info.max for r in self.near_rates):
                raise ValueError(f"near_rates must be None or 1..8 finite rates > 0, got {near_rates!r}")
            if not self.near_any_offset or self.near_top_k is None:
                raise ValueError("near_rates needs near_any_offset=True and near_top_k")
            if not _corpus_can(getattr(store, "corpus", None), "align_rates_topk", "supports_align_rates"):
                raise RuntimeError(f"near_rates={self.near_rates}: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_rates_topk; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus whose matcher has it")
        # opt-in: where the copy is (tvz_align_span_topk) - every entry gains "upload_span" and "stored_span", the first
        # and the last aligned cut on either side in seconds - and, with near_score="local", the score over that span
        # alone, which finds the copy that is partial on BOTH sides (a clip inside a compilation).  One aligned pair
        # scores 1.0 by construction, so "local" needs near_min_votes >= 2.  Neither set: nothing changes.
        self.near_spans = bool(near_spans)
        if near_score == "local" or self.near_spans:
            what = "near_score='local'" if near_score == "local" else "near_spans=True"
            if not self.near_any_offset or self.near_top_k is None:
                raise ValueError(f"{what} needs near_any_offset=True and near_top_k")
            if near_score == "local" and self.near_min_votes < 2:
                raise ValueError(f"near_score='local' needs near_min_votes >= 2 (one aligned pair scores 1.0), "
                                 f"got {near_min_votes!r}")
            if not _corpus_can(getattr(store, "corpus", None), "align_span_topk", "supports_align_span"):
                raise RuntimeError(f"{what}: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_span_topk; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus whose matcher has it")
        # opt-in: EVERY aligned part of each reported video (tvz_align_parts) - the copy with an ad put in or a scene
        # taken out aligns at two shifts, and the search reports the larger half.  After the search one call aligns the
        # upload with every reported id in full: each entry gains "parts", up to near_parts of them, each with its own
        # shift and spans, and "parts_score", the local score over all parts together.  None: nothing changes.
        self.near_parts = None if near_parts is None else int(near_parts)
        if self.near_parts is not None:
            if not 2 <= self.near_parts <= 4:
                raise ValueError(f"near_parts must be None or 2..4, got {near_parts!r}")
            if not self.near_any_offset or self.near_top_k is None or near_score != "local":
                raise ValueError(f"near_parts={self.near_parts} needs near_top_k, near_any_offset=True and near_score='local'")
            if not _corpus_can(getattr(store, "corpus", None), "align_parts", "supports_align_parts"):
                raise RuntimeError(f"near_parts={self.near_parts}: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_parts; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus whose matcher has it")
        # opt-in: the votes of a row counted over two adjacent offset bins (TVZ_ALIGN_TWO_BINS) - the copy whose shift
        # lies near a bin's edge (a remux, a re-timing to another frame grid) splits its votes over two bins and the
        # best single bin holds half of them.  The search goes through the calls that take flags: without
        # near_any_offset that is align_wide_topk with max_offset=near_max_offset (the bounded call's answer for its
        # range).  best_bin is then the window's lower bin, so shift_seconds is (best_bin + 0.5) x near_eps.
        # tvz_align_parts has no flags argument: near_parts with it is refused.  False: nothing changes.
        # near_parts_two_bins=True turns the combination with near_parts and with near_candidates ON: the parts call
        # goes through tvz_align_parts_flags with TVZ_ALIGN_TWO_BINS (align_parts(two_bins=True)), every part is a
        # window of two bins and its shift is (bin + 0.5) x near_eps.  False: refused as before.
        self.near_two_bins = bool(near_two_bins)
        self.near_parts_two_bins = bool(near_parts_two_bins)
        if self.near_parts_two_bins:
            if not self.near_two_bins or (near_parts is None and near_candidates is None):
                raise ValueError("near_parts_two_bins=True needs near_two_bins=True and near_parts or near_candidates")
            if not getattr(getattr(store, "corpus", None), "supports_align_parts_two_bins", False):
                raise RuntimeError(f"near_parts_two_bins=True: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_parts over two bins "
                                   "(supports_align_parts_two_bins); use a DeviceCorpus or a service.ShardedCorpus")
        if self.near_two_bins:
            if not near_duplicates or self.near_top_k is None:
                raise ValueError("near_two_bins=True needs near_duplicates=True and near_top_k")
            if self.near_parts is not None and not self.near_parts_two_bins:
                raise ValueError(f"near_two_bins=True with near_parts={self.near_parts}: align_parts counts single bins "
                                 "(it has no flags); use one of them")
            if not _corpus_can(getattr(store, "corpus", None), "align_wide_topk", "supports_align_wide"):
                raise RuntimeError(f"near_two_bins=True: the store's corpus "
                                   f"({type(getattr(store, 'corpus', None)).__name__}) has no align_wide_topk; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus")
        # opt-in: the search at any shift WITHOUT the sweep over every row - the near_candidates stored videos that share
        # the most gap codes with the upload (tvz_align_candidates over the corpus's gap index of near_gap_eps seconds,
        # turned on here, once) are aligned in full by one align_parts call, and the report is made from its part 0 with
        # the same score, thresholds and order as the sweep's.  Codes are made at rate 1 and the parts call counts single
        # bins: refused with near_rates and near_two_bins (the latter unless near_parts_two_bins turns the parts call's
        # flag on, above).  An upload the candidates call refuses (more than 514 cuts) takes the configured sweep.
        # None: nothing changes.
        # near_candidate_rates=True turns the combination with near_rates ON: the stored codes stay at rate 1 and the
        # upload is probed once per rate (tvz_align_candidates_rates), the parts call aligns the named videos at the same
        # rate list and every entry carries its "rate", as the rates sweep's entries do.  False: refused as before.
        self.near_candidates = None if near_candidates is None else int(near_candidates)
        self.near_gap_eps = float(near_gap_eps)
        self.near_candidate_rates = bool(near_candidate_rates)
        if self.near_candidate_rates:
            missing = [n for n, v in (("near_candidates", near_candidates), ("near_rates", near_rates)) if v is None]
            if missing:
                raise RuntimeError(f"near_candidate_rates=True needs {' and '.join(missing)}")
        if self.near_candidates is not None:
            if not near_duplicates or self.near_top_k is None or not self.near_any_offset:
                raise ValueError(f"near_candidates={self.near_candidates} needs near_duplicates=True, near_top_k and "
                                 "near_any_offset=True")
            if not self.near_top_k <= self.near_candidates <= 64:
                raise ValueError(f"near_candidates must be None or near_top_k..64 ({self.near_top_k}..64), "
                                 f"got {near_candidates!r}")
            if not (0.0 < self.near_gap_eps <= sys.float_info.max):
                raise ValueError(f"near_gap_eps must be finite and > 0, got {near_gap_eps!r}")
            what = f"near_candidates={self.near_candidates}"
            if self.near_rates is not None and not self.near_candidate_rates:
                raise RuntimeError(f"{what} with near_rates={self.near_rates}: the gap codes are made at rate 1; "
                                   "use one of them")
            if self.near_two_bins and not self.near_parts_two_bins:
                raise RuntimeError(f"{what} with near_two_bins=True: align_parts counts single bins (it has no flags); "
                                   "use one of them")
            corpus = getattr(store, "corpus", None)
            if not (_corpus_can(corpus, "align_candidates", "supports_align_candidates") and hasattr(corpus, "set_gap_index")
                    and _corpus_can(corpus, "align_parts", "supports_align_parts")):
                raise RuntimeError(f"{what}: the store's corpus ({type(corpus).__name__}) has no align_candidates; "
                                   "use a DeviceCorpus, a service.ShardedCorpus or a service.RankCorpus over a matcher "
                                   "with `candidates`")
            if self.near_candidate_rates and not _corpus_can(corpus, "align_candidates_rates", "supports_align_candidate_rates"):
                raise RuntimeError(f"near_candidate_rates=True: the store's corpus ({type(corpus).__name__}) has no "
                                   "align_candidates_rates; use a DeviceCorpus")
            corpus.set_gap_index(self.near_gap_eps)
        # near_candidates_long=True: the ids of EVERY upload come from align_candidates_long (tvz_align_candidates_long:
        # the upload looked up in segments of 511 positions, the segments' counts summed per stored video), so an
        # upload of up to 4,095 cuts no longer takes the sweep; a longer one still does.  The rates form stays at 514
        # values: refused beside near_candidate_rates.  False: nothing changes.
        self.near_candidates_long = bool(near_candidates_long)
        if self.near_candidates_long:
            if self.near_candidates is None:
                raise RuntimeError("near_candidates_long=True needs near_candidates")
            if self.near_candidate_rates:
                raise RuntimeError("near_candidates_long=True with near_candidate_rates=True: the candidates call with "
                                   "rates takes uploads of up to 514 values; use one of them")
            corpus = getattr(store, "corpus", None)
            if not _corpus_can(corpus, "align_candidates_long", "supports_align_candidates_long"):
                raise RuntimeError(f"near_candidates_long=True: the store's corpus ({type(corpus).__name__}) has no "
                                   "align_candidates_long; use a DeviceCorpus")
        # opt-in, never the default: duplicates by the TOLERANT count (include/tvz.h tvz_find_duplicates_tol)
        # instead of the reference's exact float64 equality; the verdict, the truncation at kth and the stored
        # duplicates all follow it.  Refused here, before any upload, where the store's corpus cannot do it.
        self.match_tolerance = float(match_tolerance)
        if not (0.0 <= self.match_tolerance <= sys.float_info.max):
            raise ValueError(f"match_tolerance must be finite and >= 0, got {match_tolerance!r}")
        if self.match_tolerance > 0.0 and not getattr(getattr(store, "corpus", None), "supports_tolerance", False):
            raise RuntimeError(f"match_tolerance={self.match_tolerance}: the store's corpus "
                               f"({type(getattr(store, 'corpus', None)).__name__}) has no tolerant match; "
                               "use a DeviceCorpus or a service.ShardedCorpus")
        self.device = torch.device(device)
        self.frame_source = frame_source or s3_frame_source
        self.threshold = threshold
        self.min_match = min_match          # app.py:235
        self.pts_policy = pts_policy
        self.batch = batch
        # opt-in extra, never the verdict: shift/tolerance-aware score (tvz_align) reported in an
        # additional `near_duplicates` field the reference does not have
        self.near_duplicates = near_duplicates
        self.near_eps, self.near_max_offset, self.near_jaccard = near_eps, near_max_offset, near_jaccard
        self.analysis_results: Dict[str, dict] = {}     # app.py:28
        self.analysis_lock = threading.Lock()           # app.py:29
        self.pool = ThreadPoolExecutor(max_workers=max_workers, thread_name_prefix="analyze")
        # staging shared by every upload: two slots per worker (one being filled by its reader
        # thread, one being copied / scored) + slack; created lazily
        self.slots = SlotPool(self.device, slot_bytes=slot_bytes,
                              n_slots=n_slots if n_slots is not None else 2 * max_workers + 2)
        self._scorers: Dict[tuple, list] = {}           # idle SceneScorers by (H, W, bitdepth, frames)
        self._scorers_lock = threading.Lock()
        self._tls = threading.local()
        # optional per-phase wall-clock accounting of the driver loop (profiles/e2e_service.py)
        self.phase_seconds: Optional[Dict[str, float]] = {} if profile else None
        self._phase_lock = threading.Lock()
        # frames the scene kernels have scored over all uploads (an upload that reaches a duplicate
        # verdict stops there, app.py:249-255): what a throughput figure must count, not uploads x frames
        self.frames_scored = 0

    def _phase(self, name: str, t0: float) -> float:
        t1 = time.perf_counter()
        if self.phase_seconds is not None:
            with self._phase_lock:
                self.phase_seconds[name] = self.phase_seconds.get(name, 0.0) + (t1 - t0)
                self.phase_seconds["n_" + name] = self.phase_seconds.get("n_" + name, 0) + 1
                self.phase_seconds["max_" + name] = max(self.phase_seconds.get("max_" + name, 0.0), t1 - t0)
        return t1

    def close(self) -> None:
        self.pool.shutdown(wait=True)
        self.slots.close()
        with self._scorers_lock:
            self._scorers.clear()

    def _scorer_get(self, H: int, W: int, bitdepth: int, frames: int) -> "scene.SceneScorer":
        key = (H, W, bitdepth, frames)
        with self._scorers_lock:
            idle = self._scorers.get(key)
            sc = idle.pop() if idle else None
        if sc is None:
            sc = scene.SceneScorer(H, W, frames, self.device, self.threshold, keep_scores=False,
                                   bitdepth=bitdepth)
        sc.threshold = self.threshold
        sc.reset()
        return sc, key

    def _scorer_put(self, key: tuple, sc) -> None:
        with self._scorers_lock:
            idle = self._scorers.setdefault(key, [])
            if len(idle) < 64:
                idle.append(sc)

    # ------------------------------------------------------------------ driver
    def submit(self, bucket: str, key: str):
        return self.pool.submit(self.analyze_file, bucket, key)

    def analyze_file(self, bucket: str, key: str) -> dict:
        filename, original_filename = split_filenames(key)
        unique_id = f"{int(time.time())}_{uuid.uuid4().hex[:8]}"           # app.py:134
        analysis_key = f"{unique_id}_{filename}"                           # app.py:136
        with self.analysis_lock:
            self.analysis_results.pop(analysis_key, None)
        t = time.perf_counter()
        local_path = None
        reader = None
        try:
            # inside the try: a failure here is this upload's `status: error` (app.py:303), not a
            # dead worker with no record
            if hasattr(self.store, "sync_if_stale"):
                self.store.sync_if_stale(min_interval=1.0)   # rows written by another process since our last look
            t = self._phase("sync_census", t)
            video = self.store.add_video(original_filename)                # app.py:150
            t = self._phase("add_video", t)
            video_id = video.id
            self._set(analysis_key, {"status": "analyzing", "scene_cuts": [], "progress": 0.0,
                                     "total_cuts": 0, "duplicates": [], "original_filename": filename,
                                     "clean_filename": original_filename})
            reader, local_path = self.frame_source(bucket, key, filename, unique_id)
            t = self._phase("open_source", t)
            scene_timestamps, dups_to_report = self._run(analysis_key, video_id, reader)
            t = self._phase("run_total", t)
            result = {"status": "done", "scene_cuts": scene_timestamps, "progress": 1.0,
                      "total_cuts": len(scene_timestamps),
                      "duplicates": list(set(dups_to_report)) if dups_to_report else [],
                      "original_filename": filename, "clean_filename": original_filename}
            if self.near_duplicates:
                result["near_duplicates"] = self._near(video_id, scene_timestamps)
            self._set(analysis_key, result)                                # app.py:294-302
        except Exception as e:                                             # app.py:303-315
            with self.analysis_lock:
                existing = self.analysis_results.get(analysis_key, {}).get("duplicates", [])
                result = {"status": "error", "error": str(e), "progress": 0.0, "total_cuts": 0,
                          "duplicates": existing, "original_filename": filename,
                          "clean_filename": original_filename}
                self.analysis_results[analysis_key] = result
        finally:                                                           # app.py:316-322
            if reader is not None:
                try:
                    reader.close()
                except Exception:
                    pass
            if local_path and os.path.exists(local_path):
                try:
                    os.remove(local_path)
                except Exception:
                    pass
        return result

    def _set(self, analysis_key: str, value: dict) -> None:
        with self.analysis_lock:
            self.analysis_results[analysis_key] = value

    def _run(self, analysis_key: str, video_id: int, reader):
        """GPU restatement of the hot loop app.py:216-291."""
        time_base = reader.time_base
        total_frames = getattr(reader, "total_frames", 0) or 0
        bitdepth = getattr(reader, "bitdepth", 8)
        pts_of = getattr(reader, "pts_of", None)
        frames_per_batch = self.slots.frames_per_slot(reader.H, reader.W, 1 if bitdepth == 8 else 2,
                                                      self.batch)
        # every worker thread drives its own HIP stream: uploads overlap on the GPU instead of
        # queueing behind each other on the default stream
        stream = getattr(self._tls, "stream", None)
        if stream is None:
            stream = self._tls.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(stream):
            t = time.perf_counter()
            scorer, skey = self._scorer_get(reader.H, reader.W, bitdepth, frames_per_batch)
            feeder = FrameFeeder(reader, frames_per_batch, self.device, pool=self.slots)
            self._phase("setup", t)
            scene_timestamps, dups_to_report = self._loop(analysis_key, video_id, feeder, scorer, skey,
                                                          pts_of, time_base, total_frames)
        return scene_timestamps, dups_to_report

    def _loop(self, analysis_key, video_id, feeder, scorer, skey, pts_of, time_base, total_frames):
        scene_timestamps: List[float] = []
        dups_to_report: List[str] = []
        frames_done = 0
        try:
            t = time.perf_counter()
            batches = iter(feeder)
            while True:
                try:
                    base, d_frames = next(batches)
                except StopIteration:
                    t = self._phase("wait_eof", t)
                    break
                t = self._phase("wait_frames", t)
                scorer.score_batch(d_frames)               # state (prev frame, prev mafd) stays in HBM
                t = self._phase("enqueue_score", t)
                idx = scorer.fetch_cuts()                  # the batch's ONE device-to-host sync
                t = self._phase("fetch_cuts", t)
                frames_done = base + d_frames.shape[0]
                grew = False
                for i in idx:
                    n = base + i
                    # showinfo prints pts * time_base (app.py:230): the frame's real pts
                    ts = scene.pts_time_value(pts_of(n) if pts_of else n, time_base, self.pts_policy)
                    if not scene_timestamps or ts != scene_timestamps[-1]:              # app.py:231
                        scene_timestamps.append(ts)
                        grew = True
                if grew:
                    scene_timestamps, stop = self._after_cuts(analysis_key, video_id, scene_timestamps, frames_done,
                                                              total_frames, dups_to_report)
                    t = time.perf_counter()                # (phases "match" / "persist" are timed inside)
                    if stop:
                        break                                                             # :249-255
                self._progress(analysis_key, scene_timestamps, frames_done, total_frames, dups_to_report)
                t = self._phase("progress", t)
        finally:
            with self._phase_lock:
                self.frames_scored += frames_done
            t = time.perf_counter()
            feeder.close()                                 # stops the decoder (app.py:249-252)
            self._scorer_put(skey, scorer)
            t = self._phase("close_feeder", t)
            if hasattr(self.store, "flush"):
                self.store.flush(video_id)                 # the SQL row is committed before `done`
            self._phase("flush_sql", t)
        return scene_timestamps, dups_to_report

    def _after_cuts(self, analysis_key, video_id, scene_timestamps, frames_done, total_frames, dups_to_report):
        """The reference's per-cut body (app.py:234-255) for a micro-batch that grew the cut list:
        one match over the whole current list - kth tells on which prefix the per-cut loop would
        have stopped -, persist, and on the first hit: truncate, record the duplicates, stop.
        -> (scene_timestamps, stop).  `dups_to_report` is extended in place."""
        t = time.perf_counter()
        if self.match_tolerance > 0.0:
            hits = self.store.find_duplicates_kth(scene_timestamps, self.min_match, exclude_id=video_id,
                                                  tolerance=self.match_tolerance)
        else:
            hits = self.store.find_duplicates_kth(scene_timestamps, self.min_match, exclude_id=video_id)   # :235-237
        t = self._phase("match", t)
        hits = [h for h in hits if h[2] < KTH_NEVER]
        if hits:
            kstar = min(h[2] for h in hits)
            dup_ids = [h[0] for h in hits if h[2] == kstar]
            scene_timestamps = scene_timestamps[:max(kstar, 0) + 1]
            self._persist(video_id, scene_timestamps)                                 # :234
            self.store.update_duplicates(video_id, dup_ids)                           # :239
            for dup_id in dup_ids:                                                    # :241-245
                dup_video = self.store.get_video_by_id(dup_id)
                if dup_video:
                    dups_to_report.append(dup_video.filename)
            self._progress(analysis_key, scene_timestamps, frames_done, total_frames, dups_to_report)
            self._phase("persist", t)
            return scene_timestamps, True
        self._persist(video_id, scene_timestamps)                                     # :234
        self._phase("persist", t)
        return scene_timestamps, False

    def _persist(self, video_id: int, scene_timestamps) -> None:
        """app.py:234: the growing prefix goes to the device corpus at once (the next match of any
        upload sees it) and to SQL through the store's coalescing write-behind."""
        if hasattr(self.store, "add_timestamps_async"):
            self.store.add_timestamps_async(video_id, scene_timestamps)
        else:
            self.store.add_timestamps(video_id, scene_timestamps)

    def _near(self, video_id: int, scene_timestamps):
        """Rows whose cut pattern aligns with this video's under a constant shift (tolerant Jaccard
        >= near_jaccard).  Extra field; the exact `duplicates` verdict is untouched."""
        out = []
        if len(scene_timestamps) < 2:
            return out
        rows, rated, half = self._near_search(video_id, scene_timestamps)
        local = self.near_score == "local"
        cuts = None                                                            # the upload's non-NaN cuts, sorted
        for vid, row_len, best_bin, votes, *more in rows:
            if vid == video_id or row_len == 0:
                continue
            spanned = len(more) == 4                                           # (rate_index, t_first, t_last, nr)
            if local and not spanned:                                          # (the walk has no span: no local score)
                continue
            # votes counts (query, row) pairs: cuts closer than eps can give more than either list holds
            v = min(int(votes), len(scene_timestamps), int(row_len))
            jacc = v / float(len(scene_timestamps) + row_len - v)
            if local:                                                          # the two sides inside the span
                nq, nr = int(more[2]) - int(more[1]) + 1, int(more[3])
                v = min(int(votes), nq, nr)
            if v < self.near_min_votes and self.near_min_votes > 1:
                continue
            contain = self.near_score == "containment"
            score = v / float(nq + nr - v) if local else v / float(min(len(scene_timestamps), row_len)) if contain else jacc
            if score >= self.near_jaccard:
                v = self.store.get_video_by_id(int(vid))
                out.append({"filename": v.filename if v else None, "video_id": int(vid),
                            "shift_seconds": (float(best_bin) + half) * self.near_eps, "jaccard": round(jacc, 4)})
                if contain or local:
                    out[-1][self.near_score] = round(score, 4)
                if rated:                                                      # stored ~= rate x upload + shift
                    out[-1]["rate"] = self.near_rates[int(more[0])]
                if spanned:
                    if cuts is None:
                        cuts = np.sort(np.asarray(scene_timestamps, dtype=np.float64))
                        cuts = cuts[~np.isnan(cuts)]
                    rate = self.near_rates[int(more[0])] if rated else 1.0
                    first, last = float(cuts[int(more[1])]), float(cuts[int(more[2])])
                    out[-1]["upload_span"] = [first, last]
                    out[-1]["stored_span"] = [rate * first + out[-1]["shift_seconds"], rate * last + out[-1]["shift_seconds"]]
        if self.near_parts is not None and out:
            self._near_parts(out, scene_timestamps)
        by = self.near_score if self.near_score in ("containment", "local") else "jaccard"
        return sorted(out, key=lambda d: (-d[by], d["video_id"]))

    def _near_parts(self, out, scene_timestamps) -> None:
        """near_parts: ONE align_parts call for the reported ids; every entry whose pair was not refused gains "parts" -
        per part the shift, the spans (as "upload_span" / "stored_span" are made) and the raw votes - and
        "parts_score": with v = the sum of min(votes_i, nq_i, nr_i), v / (sum nq_i + sum nr_i - v).
        near_parts_two_bins: the call counts over two bins, and a part's shift is its window's middle."""
        rates = self.near_rates or (1.0,)
        half = 0.5 if self.near_parts_two_bins else 0.0
        kept = getattr(self._tls, "candidate_parts", None) if self.near_candidates is not None else None
        if kept is not None:                                                   # near_candidates: the search's own parts block
            blocks = [kept[d["video_id"]] for d in out]
        else:
            blocks = self.store.corpus.align_parts([scene_timestamps], [[d["video_id"] for d in out]], eps=self.near_eps,
                                                   rates=rates, min_votes=self.near_min_votes, max_parts=self.near_parts,
                                                   **self._parts_two_bins())[0]
        cuts = np.sort(np.asarray(scene_timestamps, dtype=np.float64))
        cuts = cuts[~np.isnan(cuts)]
        for d, block in zip(out, blocks):
            n = int(block[0][3])
            if n < 0:                                                          # a refused pair: the entry stays as it is
                continue
            rate, parts, v, u = rates[int(block[0][2])], [], 0, 0
            for best_bin, votes, t_first, t_last, nq, nr in (tuple(int(x) for x in p) for p in block[1:1 + n]):
                shift, first, last = (float(best_bin) + half) * self.near_eps, float(cuts[t_first]), float(cuts[t_last])
                parts.append({"shift_seconds": shift, "upload_span": [first, last],
                              "stored_span": [rate * first + shift, rate * last + shift], "votes": votes})
                v += min(votes, nq, nr)
                u += nq + nr
            d["parts"] = parts
            d["parts_score"] = round(v / float(u - v), 4) if u > v else 0.0

    def _parts_two_bins(self) -> dict:
        """what near_parts_two_bins adds to an align_parts call (told only where it is set)"""
        return {"two_bins": True} if self.near_parts_two_bins else {}

    def _near_candidates(self, video_id: int, scene_timestamps):
        """near_candidates: the rows _near filters, made without a sweep - ONE align_candidates call names the stored
        videos that share the most gap codes with the upload, ONE align_parts call aligns them in full, and part 0 of
        every pair is what the span search reports for that row: (video_id, row_len, best_bin, votes, rate_index,
        t_first, t_last, nr).  The same fixed-point score, thresholds and order as the sweep keeps its rows by, the
        near_top_k best.  Rows of four columns where the configuration's sweep reports no span.  None: the candidates
        call refused the upload.  The parts block stays with the calling thread for _near_parts.
        near_candidates_long: the ids come from ONE align_candidates_long call, which refuses an upload only above 4,095
        values.
        near_candidate_rates: the ids come from ONE align_candidates_rates call with near_rates, the parts call aligns at
        the same list, and the rate_index of a row is the parts header's (rows of five columns without spans)."""
        from .corpus import align_span_order_key
        corpus = self.store.corpus
        rates = self.near_rates if self.near_candidate_rates else (1.0,)
        if self.near_candidate_rates:
            ids, _, _, totals = corpus.align_candidates_rates([scene_timestamps], rates=rates, c=self.near_candidates,
                                                              exclude_ids=[int(video_id)])
            ids = ids[0]
        else:
            call = corpus.align_candidates_long if self.near_candidates_long else corpus.align_candidates
            ids, totals = call([scene_timestamps], c=self.near_candidates, exclude_ids=[int(video_id)])
            ids = ids[0][:, 0]
        if int(totals[0]) == -(1 << 31):
            return None
        ids = [int(v) for v in ids if v >= 0]
        if not ids:
            return []
        blocks = corpus.align_parts([scene_timestamps], [ids], eps=self.near_eps, rates=rates, min_votes=self.near_min_votes,
                                    max_parts=self.near_parts or 1, **self._parts_two_bins())[0]
        one = 1 << 20
        min_score = max(0, min(one, int(self.near_jaccard * one)))
        contain, local = self.near_score == "containment", self.near_score == "local"
        spans = self.near_spans or local
        rows, kept = [], {}
        for block in blocks:
            vid, row_len, rate, n_parts, _, m = (int(x) for x in block[0])
            if n_parts < 1:                                                    # refused, no row of the id, or no part
                continue
            best_bin, votes, t_first, t_last, _, nr = (int(x) for x in block[1])
            row = (vid, row_len, best_bin, votes, rate, t_first, t_last, nr)
            key = align_span_order_key(row, m, contain=contain, local=local)
            if -key[0] >= min_score:
                rows.append((key, row))
                kept[vid] = block
        rows.sort()
        self._tls.candidate_parts = kept
        return [row if spans else row[:5 if self.near_candidate_rates else 4] for _, row in rows[:self.near_top_k]]

    def _near_rows(self, video_id: int, scene_timestamps):
        """_near_search's (rows, rated)."""
        return self._near_search(video_id, scene_timestamps)[:2]

    def _near_search(self, video_id: int, scene_timestamps):
        """(video_id, row_len, best_bin, votes[, ...]) of the rows _near filters: every row of the table (near_top_k None), or
        the near_top_k best-aligned ones, selected on the device with min_score = floor(near_jaccard x 2^20) - a
        superset of the float filter, since v / u >= j implies floor(v 2^20 / u) >= floor(j 2^20).  -> (rows, rated,
        half): rated where the fifth column is the index of the row's rate in near_rates (tvz_align_rates_topk); rows
        of eight columns carry the span behind it (tvz_align_span_topk); half = 0.5 where best_bin is the lower bin of
        a window of two (near_two_bins), so the shift is (best_bin + half) x near_eps, and 0.0 otherwise."""
        corpus = self.store.corpus
        if self.near_candidates is not None:
            self._tls.candidate_parts = None
            rows = self._near_candidates(video_id, scene_timestamps)
            if rows is not None:                                               # (None: refused -> the configured sweep)
                return rows, self.near_candidate_rates, 0.5 if self.near_parts_two_bins else 0.0
        if self.near_top_k is not None:
            one = 1 << 20
            min_score = max(0, min(one, int(self.near_jaccard * one)))          # int() floors: the value is >= 0
            rated = self.near_rates is not None
            contain, local = self.near_score == "containment", self.near_score == "local"
            # the method and what only it takes; the bounded call is told min_votes only where it is above 1
            kw = dict(max_offset=None, min_votes=self.near_min_votes, contain=contain)
            if self.near_spans or local:
                call, kw = corpus.align_span_topk, dict(kw, rates=self.near_rates or (1.0,), local=local)
            elif rated:
                call, kw = corpus.align_rates_topk, dict(kw, rates=self.near_rates)
            elif self.near_any_offset:
                call = corpus.align_wide_topk
            else:
                # (with near_two_bins: the call that takes flags, over the bounded range)
                call = corpus.align_wide_topk if self.near_two_bins else corpus.align_topk
                kw = dict(max_offset=self.near_max_offset)
                if self.near_min_votes > 1:
                    kw["min_votes"] = self.near_min_votes
            if self.near_two_bins:                                             # (told only where it is set)
                kw["two_bins"] = True
            rows, totals = call([scene_timestamps], eps=self.near_eps, k=self.near_top_k, min_score=min_score,
                                exclude_ids=[int(video_id)], **kw)
            if int(totals[0]) >= 0:                                            # (refused: more than 4,095 cuts -> the walk)
                return [r for r in rows[0] if r[0] >= 0], rated, 0.5 if self.near_two_bins else 0.0
            if not hasattr(corpus, "align"):                                   # (a rank corpus has no walk: no report)
                return [], False, 0.0
        return corpus.align(scene_timestamps, eps=self.near_eps, max_offset=self.near_max_offset), False, 0.0

    def _progress(self, analysis_key, scene_timestamps, frames_done, total_frames, dups_to_report):
        if total_frames > 0 and frames_done > 0:                           # app.py:259-260
            progress = min(frames_done / total_frames, 1.0)
        elif scene_timestamps:                                             # app.py:261-264
            estimated_duration = max(scene_timestamps) + 10
            progress = min(len(scene_timestamps) * 10 / estimated_duration, 1.0)
        else:
            progress = 0.0
        with self.analysis_lock:                                           # app.py:276-282
            rec = self.analysis_results[analysis_key]
            rec["progress"] = progress
            rec["scene_cuts"] = list(scene_timestamps)
            if dups_to_report:
                rec["duplicates"] = list(set(dups_to_report))

    # ------------------------------------------------------------------ lookup
    def result_for(self, filename: str) -> Optional[dict]:
        """app.py:72-84: exact key first, then by original_filename."""
        with self.analysis_lock:
            if filename in self.analysis_results:
                return dict(self.analysis_results[filename])
            for _, data in self.analysis_results.items():
                if isinstance(data, dict) and data.get("original_filename") == filename:
                    return dict(data)
        return None


def create_app(inspector: Inspector, sse_period: float = 0.2):
    """Flask app with the reference's routes and JSON shapes (app.py:12-115, 324-415)."""
    from flask import Flask, Response, jsonify, request

    app = Flask(__name__)

    def add_cors_headers(response):                                        # app.py:15-19
        response.headers["Access-Control-Allow-Origin"] = "*"
        response.headers["Access-Control-Allow-Methods"] = "GET, POST, OPTIONS"
        response.headers["Access-Control-Allow-Headers"] = "Content-Type"
        return response

    app.after_request(add_cors_headers)

    @app.route("/status/stream/<filename>", methods=["OPTIONS"])          # app.py:23-25
    def status_stream_options(filename):
        return add_cors_headers(Response())

    @app.route("/notify", methods=["POST"])                               # app.py:31-44
    def notify():
        data = request.get_json(silent=True)
        try:
            record = data["Records"][0]
            bucket = record["s3"]["bucket"]["name"]
            key = record["s3"]["object"]["key"]
        except Exception as e:
            return jsonify({"error": "Invalid event format", "details": str(e)}), 400
        inspector.submit(bucket, key)
        return jsonify({"status": "Analysis started", "file": key})

    @app.route("/status/<filename>", methods=["GET"])                     # app.py:46-62
    def status(filename):
        result = inspector.result_for(filename)
        if not result:
            return jsonify({"status": "pending"})
        return jsonify(result)

    @app.route("/status/stream/<filename>")                               # app.py:64-115
    def status_stream(filename):
        def event_stream():
            last = None
            while True:
                result = inspector.result_for(filename)
                if not result:
                    cur = ("pending", 0.0, 0, 0)
                else:
                    cur = (result.get("status"), result.get("progress", 0.0),
                           len(result.get("scene_cuts", [])), len(result.get("duplicates", [])))
                if cur != last:
                    last = cur
                    data = result if result else {"status": "pending"}
                    yield f"data: {json.dumps(data)}\n\n"
                    if cur[0] in ("done", "error"):
                        break
                time.sleep(sse_period)
        return add_cors_headers(Response(event_stream(), mimetype="text/event-stream"))

    @app.route("/admin/clear-db", methods=["POST"])                       # app.py:325-333
    def clear_db():
        inspector.store.clear()
        return jsonify({"status": "cleared"})

    @app.route("/build-info", methods=["GET"])                            # app.py:335-345
    def build_info():
        return jsonify({"inspector": {"build_date": os.environ.get("BUILD_DATE", "unknown"),
                                      "build_time": os.environ.get("BUILD_TIME", "unknown"),
                                      "git_commit": os.environ.get("GIT_COMMIT", "unknown"),
                                      "service": "inspector"}})

    @app.route("/debug/videos", methods=["GET"])                          # app.py:347-366
    def debug_videos():
        vids = inspector.store.list_videos()
        return jsonify({"videos": vids, "count": len(vids)})

    @app.route("/debug/create-test-video", methods=["POST"])              # app.py:368-384
    def create_test_video():
        body = request.get_json(silent=True) or {}
        test_filename = body.get("filename", "test_video.mp4")
        test_timestamps = body.get("timestamps", [1.2, 5.7, 12.3, 18.9, 25.1])
        try:
            video = inspector.store.add_video(test_filename)
            inspector.store.add_timestamps(video.id, test_timestamps)
            return jsonify({"status": "created", "video_id": video.id, "filename": test_filename,
                            "timestamps": test_timestamps})
        except Exception as e:
            return jsonify({"error": str(e)}), 500

    @app.route("/debug/analysis-results", methods=["GET"])                # app.py:386-393
    def debug_analysis_results():
        with inspector.analysis_lock:
            return jsonify({"analysis_results": inspector.analysis_results,
                            "count": len(inspector.analysis_results)})

    @app.route("/debug/test-duplicate", methods=["POST"])                 # app.py:395-415
    def test_duplicate_scenario():
        first_video = inspector.store.add_video("test.mp4")
        inspector.store.add_timestamps(first_video.id, [1.2, 5.7, 12.3, 18.9])
        second_filename = f"{int(time.time() * 1000)}-test.mp4"
        dups = inspector.store.find_duplicates([1.2, 5.7, 12.3, 18.9], min_match=2)
        return jsonify({"first_video_id": first_video.id, "second_filename": second_filename,
                        "duplicates_found": dups,
                        "message": f"Created test video, then tested duplicate detection for {second_filename}"})

    return app


def main():  # pragma: no cover - service entry point (app.py:482-484)
    from . import db
    inspector = Inspector(db.store())
    create_app(inspector).run(host="0.0.0.0", port=5000, threaded=True)


if __name__ == "__main__":  # pragma: no cover
    main()
