"""`python -m tvidz_amd.service --ranks 1 --near-top-k 16 --near-any-offset --near-score local --near-min-votes 2
--near-candidates 32 --near-rates 1.0,0.96 --near-candidate-rates` as the launcher runs it on one GPU: it starts (the
switches pass check_near_switches, reach the rank process and its Inspector), and a copy slowed down by 25/24 - stored =
0.96 x upload + shift - is reported through /notify with its rate.  One fresh rank process; only the frame source is
synthetic (tests/gap_candidates_rates_launch_parts.py)."""
import os
import threading
import time

import pytest

from tvidz_amd import service

pytestmark = pytest.mark.gpu


def test_the_launcher_starts_with_the_switch_and_reports_a_slowed_copy_with_its_rate(tmp_path):
    import requests
    from werkzeug.serving import make_server

    port = 6400 + os.getpid() % 200
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    svc = service.RankService(1, f"sqlite:///{tmp_path}/t.db", base_port=port,
                              parts="tests.gap_candidates_rates_launch_parts:rank_parts", k=16, cap=1024, workers=4,
                              ready_timeout=240, env={"PYTHONPATH": root}, near_top_k=16, near_eps=0.05, near_any_offset=True,
                              near_score="local", near_min_votes=2, near_candidates=32, near_gap_eps=0.0371,
                              near_rates="1.0,0.96", near_candidate_rates=True)
    srv = make_server("127.0.0.1", port, service.create_front(svc.urls), threaded=True)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    base = f"http://127.0.0.1:{port}"
    try:
        def key(name, pts0, cuts, stamp):
            return f"videos/{stamp}-{name}__{pts0}__{'_'.join(map(str, cuts))}.y4m"

        def upload(k, timeout=120):
            r = requests.post(f"{base}/notify", timeout=30,
                              json={"Records": [{"s3": {"bucket": {"name": "videos"}, "object": {"key": k}}}]})
            assert r.status_code == 200, r.text
            fn, end = k.split("/")[-1], time.time() + timeout
            while time.time() < end:
                rec = requests.get(f"{base}/status/{fn}", timeout=30).json()
                if rec.get("status") in ("done", "error"):
                    return rec
                time.sleep(0.05)
            raise AssertionError(f"{fn} never finished")

        # the film: cuts at multiples of 24 frames; its copy slowed by 25/24: the same cuts at multiples of 25, and moved
        film = [24, 72, 96, 144, 192, 264, 288, 336]
        copy = [c * 25 // 24 for c in film]
        other = [31, 80, 131, 170, 229, 250, 301, 377]
        first = upload(key("film", 1000, film, 1700000000))
        assert first["status"] == "done" and first["total_cuts"] == 8 and first["near_duplicates"] == [], first
        rec = upload(key("stranger", 3000, other, 1700000020))
        assert rec["status"] == "done" and rec["near_duplicates"] == [], rec
        rec = upload(key("film_slowed", 5000, copy, 1700000050))
        assert rec["status"] == "done" and rec["total_cuts"] == 8 and rec["duplicates"] == [], rec
        assert len(rec["near_duplicates"]) == 1, rec
        near = rec["near_duplicates"][0]
        assert near["rate"] == 0.96 and abs(near["shift_seconds"] - (1000 - 0.96 * 5000) / 30) < 0.05, near
        info = requests.get(f"{base}/ranks", timeout=30).json()["ranks"][0]
        assert info["rows"] == 3 and info["broken"] is None and svc.dead() == []
    finally:
        srv.shutdown()
        svc.stop()
