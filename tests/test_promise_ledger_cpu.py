"""CPU: the state machine of the no-fallback promise (adi_thermal_fields_amd/_ledger.py, bit 2 of `sparse`) on a CPU work
buffer, with the capture predicate and the read-back injected.  Both Python hosts (adi3d_hip_coeff, dist_slab.HipEngine) keep
their promises in this one class."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adi_thermal_fields_amd import _ledger, _lib  # noqa: E402
from adi_thermal_fields_amd._ledger import PromiseLedger  # noqa: E402

TG = 0.5 * 60.0                  # an ordinary theta * gamma


def work_buffer(word):
    w = torch.zeros(64, dtype=torch.uint8)
    w[:4].view(torch.int32)[0] = word
    return w


class Host:
    """a ledger with a counted read-back and a switchable capture state, used the way both hosts use it: the key only when
    the call is eligible, then bit, (call,) learn"""

    def __init__(self):
        self.reads, self.capturing = 0, False
        self.ledger = PromiseLedger(capturing=lambda: self.capturing, read_word=self.read)

    def read(self, work):
        self.reads += 1
        return _ledger._queue_word(work)

    def use(self, key, work, sp=1, tg=TG, plain=True, version=None):
        key = key if self.ledger.eligible(sp, work, tg, plain) else None
        bit = self.ledger.bit(key)
        self.ledger.learn(key, work, version)
        return bit


def test_learn_after_is_three():
    assert PromiseLedger.LEARN_AFTER == 3


@pytest.mark.parametrize('word, state, bit', [(0, True, 4), (5, False, 0)])
def test_third_use_reads_back_and_decides_for_good(word, state, bit):
    h, w = Host(), work_buffer(word)
    assert h.use('k', w) == 0 and h.ledger['k'] == 1 and h.reads == 0
    assert h.use('k', w) == 0 and h.ledger['k'] == 2 and h.reads == 0
    assert h.use('k', w) == 0                     # the third use still runs without the bit: it is the one that is read
    assert h.reads == 1 and h.ledger['k'] is state
    w[:4].view(torch.int32)[0] = 5 - word          # what the queue holds later changes nothing
    for _ in range(3):
        assert h.use('k', w) == bit
    assert h.reads == 1 and h.ledger['k'] is state
    assert h.use('other', w) == 0 and h.ledger['other'] == 1      # per configuration


INELIGIBLE = {
    'dense_reads': dict(sp=2),
    'no_workspace': dict(work=None),
    'workspace_below_one_word': dict(work=torch.zeros(3, dtype=torch.uint8)),
    'below_the_gate': dict(tg=float(np.nextafter(_lib.MIXED_MIN_TG, 0.0))),
    'axis2_with_interface_values': dict(plain=False),
}


@pytest.mark.parametrize('name', sorted(INELIGIBLE))
def test_an_ineligible_call_neither_learns_nor_carries(name):
    h, w = Host(), work_buffer(0)
    kw = dict(work=w)
    kw.update(INELIGIBLE[name])
    for _ in range(4):                             # never learns
        assert h.use('k', **kw) == 0
    assert len(h.ledger) == 0 and h.reads == 0
    for _ in range(3):
        h.use('k', w)
    assert h.ledger['k'] is True and h.use('k', w) == 4
    before = dict(h.ledger)
    assert h.use('k', **kw) == 0                   # never carries, even what is already learnt
    assert dict(h.ledger) == before and h.reads == 1
    assert h.use('k', w) == 4


def test_the_gate_is_inclusive():
    h, w = Host(), work_buffer(0)
    assert PromiseLedger.eligible(1, w, _lib.MIXED_MIN_TG)
    assert PromiseLedger.eligible(3, w, _lib.MIXED_MIN_TG)        # the all-solid hint (bit 1) does not matter
    assert not PromiseLedger.eligible(1, w, float('nan'))
    for _ in range(3):
        h.use('k', w, tg=_lib.MIXED_MIN_TG)
    assert h.ledger['k'] is True and h.use('k', w, tg=_lib.MIXED_MIN_TG) == 4


def test_capture_counts_but_does_not_read():
    h, w = Host(), work_buffer(0)
    h.capturing = True
    for n in range(1, 6):
        assert h.use('k', w) == 0
        assert h.ledger['k'] == n and h.reads == 0
    h.capturing = False
    assert h.use('k', w) == 0                      # the first use after the capture reads
    assert h.reads == 1 and h.ledger['k'] is True
    assert h.use('k', w) == 4


def test_a_newer_mask_version_drops_the_older_entries():
    h, w = Host(), work_buffer(0)
    for _ in range(3):
        h.use(('a', 1), w, version=1)
    h.use(('b', 1), w, version=1)
    assert h.ledger == {('a', 1): True, ('b', 1): 1}              # the same version: nothing is dropped
    h.use(('a', 2), w, version=2)
    assert h.ledger == {('a', 2): 1}
    h.use(('a', 2), w, version=2)                                 # a known key prunes nothing and counts on
    assert h.ledger == {('a', 2): 2}
    assert h.use(('a', 1), w, version=1) == 0                     # the old configuration starts over
    assert h.ledger == {('a', 1): 1}


def test_clear_empties_the_table():
    h, w = Host(), work_buffer(0)
    for _ in range(3):
        h.use('k', w)
    h.use('j', w)
    assert len(h.ledger) == 2
    h.ledger.clear()
    assert len(h.ledger) == 0 and h.use('k', w) == 0 and h.ledger['k'] == 1


def test_the_default_read_back_is_the_first_word():
    assert _ledger._queue_word(work_buffer(0)) == 0
    assert _ledger._queue_word(work_buffer(7)) == 7
    led, w = PromiseLedger(capturing=lambda: False), work_buffer(7)
    for _ in range(3):
        led.learn('k', w)
    assert led['k'] is False and led.bit('k') == 0 and led.bit(None) == 0
