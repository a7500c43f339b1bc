"""The host side of the table walks without a GPU (csrc/pdog_math.cpp: check_table_walk, fill_table), as the stand-alone program
tests/table_main.cpp, plain and under AddressSanitizer and UBSan with exactly sized heap buffers: the staged words against a
NumPy restatement written here — both layouts, one and three windows per row, rows of 0, 2 and 4 of 4 steps —, the padding rule
spelled out, and the order in which a doubly wrong walk is refused."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pawsometracker.jl_amd", "csrc")
N_FRAMES = 7
TABLE = np.array([[-1, -1, -1, -1],        # no step at all
                  [5, 3, -1, -1],          # two steps
                  [1, 2, 6, 4]], np.int32)  # all four


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("table") / "table_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *request.param, "-I", CSRC,
                           os.path.join(ROOT, "tests", "table_main.cpp"), "-o", str(exe)])

    def run(table, windows, first=0, n_frames=N_FRAMES):
        p = subprocess.run([str(exe), str(n_frames), str(table.shape[0]), str(table.shape[1]), str(windows), str(first),
                            *(str(int(v)) for v in table.ravel())], capture_output=True, text=True, timeout=60)
        assert p.returncode in (0, 2), p.stdout[-2000:] + p.stderr[-2000:]       # (a sanitizer's report ends the run otherwise)
        return p.returncode, p.stdout.splitlines()
    return run


def restate(table, windows):
    """(lengths, max_len, words): the rows' leading non-negative entries; windows = 0: the rows as given; windows = T: step s's
    cells are [n_rows][T], a row's frame there row[min(s, len - 1)], frame 0 for a row without a step; the lengths behind."""
    lens = (table >= 0).cumprod(axis=1).sum(axis=1).astype(np.int32)
    max_len = int(lens.max())
    if windows == 0:
        cells = table.ravel()
    else:
        at = np.minimum(np.arange(max_len)[:, None], lens[None, :] - 1)                           # [max_len][n_rows]
        frame = np.where(lens[None, :] > 0, table[np.arange(table.shape[0])[None, :], np.maximum(at, 0)], 0)
        cells = np.repeat(frame[:, :, None], windows, axis=2).ravel()
    return lens, max_len, np.concatenate([cells, lens]).astype(np.int32)


@pytest.mark.parametrize("windows", [0, 1, 3], ids=["rows", "by_step_T1", "by_step_T3"])
def test_staged_words_equal_the_restatement(program, windows):
    rc, lines = program(TABLE, windows)
    assert rc == 0, lines
    lens, max_len, words = restate(TABLE, windows)
    assert lens.tolist() == [0, 2, 4] and max_len == 4                            # the premise
    assert lines[0] == "len 0 2 4 max 4"
    got = np.array(lines[1].split()[1:], np.int32)
    assert lines[1].startswith("words ") and np.array_equal(got, words), (got, words)
    n_rows, n_steps = TABLE.shape
    cells = n_rows * (n_steps if windows == 0 else max_len * windows)
    assert got.size == cells + n_rows and got[cells:].tolist() == [0, 2, 4]      # the lengths follow the cells
    if windows:
        by_step = got[:cells].reshape(max_len, n_rows, windows)
        assert (by_step[:, 0] == 0).all()                                         # the row without a step: frame 0 in every step
        assert [by_step[s, 1].tolist() for s in range(4)] == [[5] * windows, [3] * windows, [3] * windows, [3] * windows]   # its second frame repeats
        assert [by_step[s, 2, 0] for s in range(4)] == [1, 2, 6, 4]
    else:
        assert np.array_equal(got[:cells].reshape(TABLE.shape), TABLE)


def test_a_shorter_longest_row_shortens_the_steps(program):
    """max_len, not n_steps, counts the by-step cells: rows of 0, 2 and 1 steps stage two steps."""
    table = np.array([[-1, -1, -1, -1], [5, 3, -1, -1], [6, -1, -1, -1]], np.int32)
    rc, lines = program(table, 3)
    lens, max_len, words = restate(table, 3)
    assert rc == 0 and max_len == 2 and lines[0] == "len 0 2 1 max 2"
    assert np.array_equal(np.array(lines[1].split()[1:], np.int32), words) and words.size == 2 * 3 * 3 + 3


def test_a_wrong_walk_is_refused_in_the_entry_points_order(program):
    bad = TABLE.copy()
    bad[2, 3] = N_FRAMES
    hole = np.array([[0, -1, 1, -1]], np.int32)
    for table, windows, first, n_frames, text in (
            (TABLE, 1, 2, N_FRAMES, "table_main: first must be 0 or 1"),
            (TABLE, 1, 2, 0, "table_main: bad size/stride"),                                     # the stack before first
            (bad, 1, 2, N_FRAMES, "table_main: first must be 0 or 1"),                           # first before the table
            (bad, 3, 1, N_FRAMES, "table_main: entry 3 of clip 2 names a frame outside the stack"),
            (hole, 1, 0, N_FRAMES, "table_main: entry 2 of clip 0 follows a negative one")):
        rc, lines = program(table, windows, first, n_frames)
        assert rc == 2 and lines == ["error " + text], (lines, text)
