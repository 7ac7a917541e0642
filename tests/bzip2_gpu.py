"""What the GPU tests of the bzip2 decoder share: one launch of nx_bzip2_decode_batch over guarded output
slots, and the item-for-item comparison with nx_bzip2_decode_host."""
import torch

import bzip2_streams as S

GUARD = S.GUARD


def decode(B, dev, streams, caps):
    """One launch.  Streams are packed back to back; item i's slot has caps[i] bytes between guards of GUARD
    bytes of 0xA5 and a third of the slots start at odd addresses.  Returns (out_len, consumed, status,
    outputs) with the guards checked: on an error the slot beyond out_len may have been written, the guards not."""
    buf, offs = bytearray(), []
    for s in streams:
        offs.append(len(buf))
        buf += s
    buf += b"\x00" * 16
    ooffs, cur = [], 0
    for i, c in enumerate(caps):
        cur += GUARD + (1 if i % 3 == 1 else 0)
        ooffs.append(cur)
        cur += c
    cur += GUARD
    inp = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)
    out_len, consumed, status = B.bzip2_decode(inp, t(offs, torch.int64), t([len(s) for s in streams], torch.int32), out,
                                               t(ooffs, torch.int64), t(caps, torch.int32))
    torch.cuda.synchronize()
    outa = out.cpu().numpy()
    out_len, consumed, status = out_len.cpu().tolist(), consumed.cpu().tolist(), status.cpu().tolist()
    res = []
    for i, (o, c, w) in enumerate(zip(ooffs, caps, out_len)):
        assert 0 <= w <= c, (i, w, c)
        res.append(outa[o:o + w].tobytes())
        outa[o:o + c] = 0xA5
    changed = (outa != 0xA5).nonzero()[0]  # every byte outside the slots
    assert changed.size == 0, f"a guard byte changed, first at {int(changed[0])}"
    return out_len, consumed, status, res


def equal_host(B, streams, caps, got):
    out_len, consumed, status, res = got
    for i, (s, c) in enumerate(zip(streams, caps)):
        st, out, used = B.bzip2_decode_host(s, c)
        assert (status[i], out_len[i], consumed[i]) == (st, len(out), used), i
        if st == S.OK:
            assert res[i] == out, i
