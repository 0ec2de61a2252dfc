"""The no-fallback promise of the Python hosts: bit 2 of the `sparse` argument (include/adi_hip.h)."""
import torch

from ._lib import MIXED_MIN_TG


def _queue_word(work):
    """units the last FAST kernel queued: the first word of the sweep workspace (one 4-byte copy; synchronises the host)"""
    return int(work[:4].view(torch.int32)[0].item())


class PromiseLedger(dict):
    """configuration key -> uses so far (int), or what the queue read-back said (True: no unit queued; False: some were).

    Bit 2 of `sparse` skips the queue reset and the GENERAL launch behind a FAST kernel that is known to take every unit.
    Which units a FAST kernel queues depends on the flags, the Dirichlet mask, the variant, the `sparse` bits and the shape
    -- not on the field -- so the first sweeps of a configuration run without the bit, use LEARN_AFTER reads the number of
    queued units back, and later sweeps carry the bit when it was zero.  The read-back synchronises the host, hence not
    at the first use: a layer-birth loop that changes the mask every two or three steps (waam.run_layer_birth) never pays
    it.  WHETHER a FAST kernel runs at all depends on the call (`eligible`); a call that is not eligible leaves the queue
    word as it was, so it neither learns nor carries the bit: its host passes key None.  The hosts build their own keys
    and forget in their own way: `learn(..., version)` on a pack that outlives mask versions, `clear()` on a mask event."""
    LEARN_AFTER = 3

    def __init__(self, capturing=torch.cuda.is_current_stream_capturing, read_word=_queue_word):
        super().__init__()
        self.capturing, self.read_word, self.version = capturing, read_word, None

    @staticmethod
    def eligible(sp, work, tg, plain=True):
        """sparse reads on, a workspace that holds the queue word, tg = theta * gamma at or above the library's gate (below
        it the GENERAL kernels take the whole sweep), and `plain`: not an axis-2 sweep with interface values (xlo / xhi),
        which takes the thread-per-line kernel"""
        return bool((sp & 1) and work is not None and work.numel() >= 4 and tg >= MIXED_MIN_TG and plain)

    def clear(self):
        super().clear()
        self.version = None

    def bit(self, key):
        return 4 if key is not None and self.get(key) is True else 0

    def learn(self, key, work, version=None):
        """after the call: one more use of `key`; from use LEARN_AFTER on, outside stream capture, the queue word decides
        for good.  A new key drops the entries of every mask version but its own (a layer-birth run would otherwise add
        three keys per birth for good)."""
        st = self.get(key, 0)
        if key is None or st is True or st is False:
            return
        if st == 0 and version != self.version:       # (0: a new key)
            self.clear()
            self.version = version
        st += 1
        if st >= self.LEARN_AFTER and not self.capturing():
            st = self.read_word(work) == 0
        self[key] = st
