"""Guarded device arenas for the device-pointer (`_d`) entry points.

The host forms of the C ABI stage every array at the START of a workspace allocation, so through them a kernel only ever sees
maximally aligned pointers with slack behind its output.  A caller that keeps its data on the GPU passes
`base + k * sizeof(element)`.  An arena puts one array of a call at such a pointer and watches everything around it:

    [ lead bytes of sentinel | payload | tail bytes of sentinel ]

The whole arena is filled with a fixed, non-repeating word pattern (0xC9000000 | word index: as f32 about -5e5 -- finite, so a
sentinel read as data is a gross error and not a NaN a comparison could mask; as two words of an f64 about -3.6e43), the input is
uploaded at `base + lead`, and `base + lead` is the pointer handed out.  After the call the WHOLE arena comes back and every
byte outside the payload must still hold its sentinel; an input arena's payload must still hold the input.

`lead` is in bytes and carries the pointer phase under test (hipMalloc bases are at least 256-byte aligned, which Arena
asserts).  The tail is at least 256 bytes and ends the arena on no vector boundary.

image() / verify() are plain numpy, so the guard logic has a CPU self-test (test_dptr_host.py): a guard that cannot see a
stray store would pass everything silently.
"""
import ctypes as C

import numpy as np

SENTINEL = 0xC9000000
MIN_GUARD = 256            # bytes of sentinel in front of and behind every payload, at least


def sentinel_words(n_words):
    assert n_words < (1 << 24), "arena too large for a non-repeating sentinel"
    return np.uint32(SENTINEL) | np.arange(n_words, dtype=np.uint32)


def tail_bytes(lead, payload):
    """>= MIN_GUARD, and such that the arena ends 4 bytes past a 64-byte line: the last word sits on no 8 / 16 / 64-byte boundary"""
    t = MIN_GUARD
    while (lead + payload + t) % 64 != 4:
        t += 4
    return t


def image(lead, payload, data=None):
    """The arena as uploaded: uint32 words, sentinel everywhere, `data` (any dtype, payload bytes) at byte offset lead."""
    assert lead % 4 == 0 and payload % 4 == 0 and lead >= 0 and payload >= 0
    words = sentinel_words((lead + payload + tail_bytes(lead, payload)) // 4)
    if data is not None:
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert raw.size == payload, (raw.size, payload)
        words[lead // 4: (lead + payload) // 4] = raw.view(np.uint32)
    return words


def verify(words, lead, payload, name, data=None):
    """AssertionError unless every word outside [lead, lead + payload) still holds its sentinel (and, for an input arena, the
    payload still holds `data`).  The message counts the words hit and gives their distance from the payload."""
    words = np.asarray(words, np.uint32)
    want = sentinel_words(words.size)
    lo, hi = lead // 4, (lead + payload) // 4
    problems = []
    front = np.flatnonzero(words[:lo] != want[:lo])
    if front.size:
        d = (lo - front) * 4   # bytes from the start of the word to the start of the payload
        problems.append(f"{front.size} word(s) written IN FRONT of the payload, {int(d.min())} .. {int(d.max())} bytes before its start "
                        f"(first: word {int(front[0])} = 0x{int(words[front[0]]):08x})")
    back = np.flatnonzero(words[hi:] != want[hi:])
    if back.size:
        d = back * 4           # bytes from the end of the payload to the start of the word
        problems.append(f"{back.size} word(s) written BEHIND the payload, {int(d.min())} .. {int(d.max())} bytes past its end "
                        f"(first: 0x{int(words[hi + back[0]]):08x})")
    if data is not None:
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8).view(np.uint32)
        hit = np.flatnonzero(words[lo:hi] != raw)
        if hit.size:
            problems.append(f"{hit.size} word(s) of the INPUT were overwritten, first at byte {int(hit[0]) * 4} of the payload")
    if problems:
        raise AssertionError(f"arena '{name}' (lead {lead} = {lead % 16} mod 16, payload {payload} bytes): " + "; ".join(problems))


class Arena:
    """One array of a call on the device.  data: the input (checked to be unchanged afterwards); nbytes: an output of that many
    bytes.  phase: the pointer's offset in bytes from a 256-byte boundary (the lead is MIN_GUARD + phase)."""

    def __init__(self, ctx, name, phase, data=None, nbytes=None):
        self.ctx, self.name = ctx, name
        self.data = None if data is None else np.ascontiguousarray(data)
        self.payload = self.data.nbytes if data is not None else int(nbytes)
        self.lead = MIN_GUARD + int(phase)
        img = image(self.lead, self.payload, self.data)
        self.size = img.nbytes
        self.base = ctx.dev_alloc(self.size)
        assert self.base % 256 == 0, hex(self.base)
        ctx.call("tsdr_upload", C.c_void_p(self.base), C.c_void_p(img.ctypes.data), self.size)
        self.words = None

    @property
    def addr(self):
        return self.base + self.lead

    @property
    def ptr(self):
        return C.c_void_p(self.addr)

    def fetch(self):
        """download the whole arena (after ctx.synchronize()) and check the guards; -> self"""
        w = np.empty(self.size // 4, np.uint32)
        self.ctx.call("tsdr_download", C.c_void_p(w.ctypes.data), C.c_void_p(self.base), self.size)
        self.words = w
        verify(w, self.lead, self.payload, self.name, self.data)
        return self

    def get(self, dtype, shape=None, order="C"):
        """the payload as downloaded by fetch()"""
        a = self.words[self.lead // 4: (self.lead + self.payload) // 4].view(dtype)
        return a.copy() if shape is None else a.reshape(shape, order=order).copy(order=order)

    def free(self):
        if self.base:
            self.ctx.dev_free(self.base)
            self.base = 0


class Arenas:
    """The arenas of one call:

        with Arenas(ctx) as A:
            x, y = A.input("x", sig, 4), A.output("y", 4 * n, 12)
            ctx.call("tsdr_..._d", x.ptr, n, y.ptr)
            A.check()                       # synchronise, download everything, assert every guard
            got = y.get(np.float32)
    """

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        # (an arena is freed only after the stream has drained: a failed assertion must not free memory a kernel still uses)
        try:
            self.ctx.synchronize()
        finally:
            for a in self.all:
                a.free()
        return False

    def input(self, name, data, phase):
        a = Arena(self.ctx, name, phase, data=data)
        self.all.append(a)
        return a

    def output(self, name, nbytes, phase):
        a = Arena(self.ctx, name, phase, nbytes=nbytes)
        self.all.append(a)
        return a

    def check(self):
        self.ctx.synchronize()
        for a in self.all:
            a.fetch()
