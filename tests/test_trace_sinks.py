"""End-to-end trace upload through real sinks (VERDICT r01 missing #7).

Exercises the v2.0.0 incremental payload + uploadedIds watermark
(traceCollectorService.ts:797-899 semantics) against the FileSink and a
live Unix-domain-socket server for the UDSSink.
"""

import json
import os
import socket
import threading

from senweaver_amd.trace import TraceCollector
from senweaver_amd.trace.sinks import FileSink, UDSSink


def _mk_traces(tc, n, tag):
    for i in range(n):
        tid = tc.start_trace(f"{tag}-{i}", {"chatMode": "agent"})
        tc.record_user_message(f"{tag}-{i}", 0, f"question {i}")
        tc.record_assistant_message(f"{tag}-{i}", 1, f"answer {i}")
        tc.end_trace(tid)


def test_file_sink_incremental_watermark(tmp_path):
    tc = TraceCollector()
    _mk_traces(tc, 3, "a")
    sink = FileSink(str(tmp_path / "traces.jsonl"))
    res = tc.upload_to_sink(sink)
    assert res["success"] and res["uploadedCount"] == 3
    # second upload with nothing new: watermark holds
    res = tc.upload_to_sink(sink)
    assert res["success"] and res["uploadedCount"] == 0
    # new trace -> only the delta goes out
    _mk_traces(tc, 1, "b")
    res = tc.upload_to_sink(sink)
    assert res["uploadedCount"] == 1
    lines = (tmp_path / "traces.jsonl").read_text().strip().split("\n")
    assert len(lines) == 2  # two non-empty payload uploads
    p0 = json.loads(lines[0])
    assert p0["version"] == "2.0.0"
    assert len(p0["traces"]) == 3
    assert json.loads(lines[1])["traces"][0]["id"]  # delta payload


def test_uds_sink_end_to_end(tmp_path, monkeypatch):
    # sun_path holds ~107 bytes and pytest's tmp_path can be deeper than
    # that: bind/connect by a name relative to the temp dir instead
    monkeypatch.chdir(tmp_path)
    sock_path = "collector.sock"
    received = []
    srv = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    srv.bind(sock_path)
    srv.listen(2)

    def serve():
        for _ in range(2):
            conn, _addr = srv.accept()
            buf = b""
            while not buf.endswith(b"\n"):
                chunk = conn.recv(65536)
                if not chunk:
                    break
                buf += chunk
            received.append(json.loads(buf.decode()))
            conn.sendall(b'{"ok": true}\n')
            conn.close()

    t = threading.Thread(target=serve, daemon=True)
    t.start()

    tc = TraceCollector()
    _mk_traces(tc, 2, "u")
    sink = UDSSink(sock_path)
    res = tc.upload_to_sink(sink)
    assert res["success"] and res["uploadedCount"] == 2
    _mk_traces(tc, 1, "v")
    res = tc.upload_to_sink(sink)
    assert res["uploadedCount"] == 1
    t.join(timeout=10)
    srv.close()
    assert len(received) == 2
    assert received[0]["version"] == "2.0.0"
    assert len(received[0]["traces"]) == 2 and len(received[1]["traces"]) == 1
    # payload shape: summary fields the backend aggregates
    assert "rewardSummary" in received[0] or "summary" in received[0]["traces"][0]


def test_uds_sink_failure_keeps_watermark(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # short relative socket name, as above
    tc = TraceCollector()
    _mk_traces(tc, 2, "w")
    res = tc.upload_to_sink(UDSSink("nonexistent.sock", timeout=0.5))
    assert not res["success"]
    # nothing marked uploaded: the next (working) sink gets everything
    got = tc.upload_to_sink(FileSink(str(tmp_path / "t.jsonl")))
    assert got["uploadedCount"] == 2
