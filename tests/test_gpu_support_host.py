"""tests/gpu_support.py without a GPU: it imports without loading a shared library, and its sentinel checks
fail on exactly the buffers they are there to catch."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from gpu_support import GUARD, SENTINEL, SENTINEL_WORD, assert_all_written, assert_sentinel_after, rayleigh

REC, N, SLOTS = 32, 3, 7     # a buffer of 7 records of 32 bytes, the list is the first 3


def test_import_loads_no_shared_library():
    code = ("import conftest, gpu_support\n"
            "print([l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l or 'libfmcw' in l])")
    out = subprocess.run([sys.executable, "-c", code], cwd=str(REPO / "tests"), capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "[]", out.stdout


def written_buffer():
    raw = np.full(SLOTS * REC, SENTINEL, np.uint8)
    raw[:N * REC] = np.arange(N * REC) % 251
    return raw


def test_sentinel_tail_of_an_untouched_buffer():
    assert_sentinel_after(written_buffer(), N, REC)
    assert_sentinel_after(np.full(4, GUARD, np.uint32))


@pytest.mark.parametrize("at", [N * REC, SLOTS * REC - 1], ids=["first", "last"])
def test_sentinel_tail_fails_on_one_changed_byte(at):
    raw = written_buffer()
    raw[at] ^= 1
    with pytest.raises(AssertionError, match=f"the first at byte {at} "):
        assert_sentinel_after(raw, N, REC)


@pytest.mark.parametrize("byte", range(8))
def test_sentinel_check_fails_on_one_changed_byte_of_a_guard_word(byte):
    guard = np.full(2, GUARD, np.uint32)
    guard.view(np.uint8)[byte] = 0
    with pytest.raises(AssertionError, match=f"guard words: 1 of the 8 bytes .* the first at byte {byte} "):
        assert_sentinel_after(guard, what="guard words")


@pytest.mark.parametrize("word", [0, 5, 15], ids=["first", "middle", "last"])
def test_all_written_fails_on_one_sentinel_word(word):
    raw = (np.arange(16, dtype=np.uint32) + 1).view(np.uint8).copy()
    assert_all_written(raw, "clean")
    raw.view(np.uint32)[word] = SENTINEL_WORD
    with pytest.raises(AssertionError, match=f"1 words were never written, the first at word {word}$"):
        assert_all_written(raw, "one word left")
    # three sentinel bytes and one other are a written word
    raw[4 * word] = 0
    assert_all_written(raw, "a byte of it written")


def test_rayleigh_is_the_seeded_map_and_read_only():
    m = rayleigh(2, 8, 4, 61)
    assert m.tobytes() == np.random.default_rng(61).rayleigh(1.0, (2, 8, 4)).astype(np.float32).tobytes()
    assert m.dtype == np.float32 and not m.flags.writeable and rayleigh(2, 8, 4, 61) is m
    with pytest.raises(ValueError):
        m[0, 0, 0] = 1.0
