"""Buffer.peek_raw / SyntheticBuffer.peek_raw: the rows the next next_raw() returns, without advancing (the fused
Trainer preps them inside the running step).  On the CPU, with the golden fake LMs and torch indexing in place of
cc_gather_rows."""
import json
import os

import torch

import crosscoder_amd as ca
from tests.test_cpu_host import GOLDEN, FakeLM


def _torch_gather(src, perm, out=None):
    out = torch.empty_like(src) if out is None else out
    out.copy_(src[perm])
    return out


def _fake_lm_buffer(monkeypatch, enc_dtype):
    r = torch.load(os.path.join(GOLDEN, "buffer_fake_lm.pt"), weights_only=True)
    cfg = dict(json.loads(r["cfg"]), device="cpu", enc_dtype=enc_dtype)
    monkeypatch.setattr(ca.Buffer, "gather_rows", staticmethod(_torch_gather))
    torch.manual_seed(49)
    return ca.Buffer(cfg, FakeLM(r["A_table"], r["A_pos"]), FakeLM(r["B_table"], r["B_pos"]), r["tokens"]), len(r["next"])


def test_peek_raw_names_the_next_batch_across_refreshes(monkeypatch):
    buf, n_next = _fake_lm_buffer(monkeypatch, "bf16")
    refreshes = buf.refresh_count
    for _ in range(max(n_next, 8)):
        rows, factor = buf.peek_raw()
        assert rows.data_ptr() == buf.buffer[buf.buffer_pointer:].data_ptr()  # a view, nothing advanced
        want, count = rows.clone(), buf.refresh_count
        assert buf.peek_raw()[0].data_ptr() == rows.data_ptr()
        got, got_factor = buf.next_raw()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and got_factor is factor
        if buf.refresh_count != count:
            # that call refreshed: it returned a copy, and the next peek is already of the refreshed buffer
            assert got.data_ptr() != rows.data_ptr() and buf.buffer_pointer == 0
            assert buf.peek_raw()[0].data_ptr() == buf.buffer.data_ptr()
    assert buf.refresh_count > refreshes  # (the loop crossed a refresh boundary)


def test_peek_raw_cannot_say_for_the_fp32_batch_a_refresh_overwrites(monkeypatch):
    buf, _ = _fake_lm_buffer(monkeypatch, "fp32")
    B = buf.cfg["batch_size"]
    while buf.buffer_pointer + B <= buf.buffer.shape[0] // 2 - B:
        want = buf.peek_raw()[0].clone()
        assert torch.equal(buf.next_raw()[0], want)
    assert buf.peek_raw() is None  # next_raw() refreshes and returns rows aliasing what the refresh rewrites
    count = buf.refresh_count
    buf.next_raw()
    assert buf.refresh_count == count + 1 and buf.peek_raw() is not None


def test_synthetic_buffer_peek_raw_wraps_like_next_raw():
    cfg = {"batch_size": 8, "enc_dtype": "bf16", "d_in": 16, "device": "cpu"}
    buf = ca.SyntheticBuffer(cfg, rows=20, seed=0)
    for _ in range(6):
        rows, factor = buf.peek_raw()
        got, got_factor = buf.next_raw()
        assert got.data_ptr() == rows.data_ptr() and got.shape == rows.shape and got_factor is factor
