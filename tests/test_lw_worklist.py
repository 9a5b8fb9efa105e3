"""The incremental pass B's work on the host (csrc/long_window.hip ``long_window_work_list``
and ``long_window_shape_work``): which (segment, chunk) workgroups a refresh streams, and how
the list becomes pass B's grid. Pure functions of a few integers and host flags, so they are
checked here without a GPU; LongWindowSet calls the same functions.

Everything runs at window 1024 with 256-row chunks (4 chunks), the smallest window the class
accepts. Chunks are the device ring's slots: row r lives in slot r & 1023, chunk slot // 256."""

import pytest

W, ROWS, NCHUNKS = 1024, 256, 4
FUSE_CHUNKS, SPLIT_MAX = 4, 2048  # LongWindowSet::kFuseChunks, kSplitMax


@pytest.fixture(scope="module")
def nat():
    try:
        from rocmdash.runtime import native

        return native.load(with_torch=False)
    except Exception as e:  # noqa: BLE001 - the native build is checked by its own tests
        pytest.skip(f"native module absent: {e}")


def _list(nat, width, head, copied, want=1, changed=()):
    """One ring of `width` series whose segments all had their last pass B at `head`."""
    nseg = (width + 7) // 8
    never = nat.LONG_WINDOW_NEVER
    flags = [1 if s in changed else 0 for s in range(width)]
    wants = want if isinstance(want, list) else [want] * width
    work, heads = nat.long_window_work_list(W, [(width, ROWS, NCHUNKS, copied)], [never if head is None else head] * nseg,
                                            wants, flags)
    return work, heads


def test_never_streamed_takes_every_chunk(nat):
    work, heads = _list(nat, 4, None, 130)
    assert work == [0, 1, 2, 3]
    assert heads == [130]


def test_changed_bracket_takes_every_chunk(nat):
    work, heads = _list(nat, 4, 100, 130, changed={1})
    assert work == [0, 1, 2, 3]
    assert heads == [130]


def test_new_rows_in_one_chunk(nat):
    work, heads = _list(nat, 4, 100, 130)
    assert work == [0]
    assert heads == [130]


def test_new_rows_across_two_chunks(nat):
    assert _list(nat, 4, 250, 260)[0] == [0, 1]


def test_new_rows_wrap_tail_then_head(nat):
    work, heads = _list(nat, 4, 1000, 1030)
    assert work == [3, 0]  # slots 1000..1023, then 0..5: no duplicate
    assert heads == [1030]


def test_a_window_or_more_entered_takes_every_chunk(nat):
    assert _list(nat, 4, 100, 100 + W)[0] == [0, 1, 2, 3]
    assert _list(nat, 4, 100, 100 + W + 77)[0] == [0, 1, 2, 3]
    # one row short of the window: every chunk once, from the head's chunk around the ring
    assert _list(nat, 4, 100, 100 + W - 1)[0] == [0, 1, 2, 3]
    assert _list(nat, 4, 300, 300 + W - 1)[0] == [1, 2, 3, 0]


def test_no_new_rows_no_chunks(nat):
    work, heads = _list(nat, 4, 130, 130)
    assert work == [] and heads == [130]


def test_no_series_wants_brackets(nat):
    work, heads = _list(nat, 4, 100, 130, want=0)
    assert work == []
    assert heads == [nat.LONG_WINDOW_NEVER]  # the segment's counts go stale


def test_second_segment_only(nat):
    never = nat.LONG_WINDOW_NEVER
    want = [0] * 8 + [0, 0, 1, 0, 0]  # a 13-wide ring: columns 0-7 and 8-12
    work, heads = _list(nat, 13, None, 130, want=want)
    assert work == [(1 << 20) | c for c in range(NCHUNKS)]
    assert heads == [never, 130]
    work, heads = nat.long_window_work_list(W, [(13, ROWS, NCHUNKS, 160)], heads, want, [0] * 13)
    assert work == [(1 << 20) | 0] and heads == [never, 160]


def test_two_rings_number_segments_and_series_in_order(nat):
    # ring 0: 13 series (segments 0, 1), ring 1: 2 series (segment 2, series 13-14)
    want = [0] * 13 + [0, 1]
    work, heads = nat.long_window_work_list(W, [(13, ROWS, NCHUNKS, 130), (2, ROWS, NCHUNKS, 700)], [100, 100, 500], want,
                                            [0] * 15)
    assert work == [(2 << 20) | 1, (2 << 20) | 2]
    assert heads == [nat.LONG_WINDOW_NEVER, nat.LONG_WINDOW_NEVER, 700]


# Shaping. Four segments of 2, 2, 1 and 1 columns (flat grid 4 x 4 = 16): one changed chunk in
# segment 0, all four chunks of segment 1.
SEG_COLS = [2, 2, 1, 1]
FLAT = NCHUNKS * len(SEG_COLS)
LIST = [(0 << 20) | 2] + [(1 << 20) | c for c in range(NCHUNKS)]


def _split(seg, chunk, ncols):
    return [(seg << 23) | (col << 20) | chunk for col in range(ncols)]


def test_shape_fuse_on(nat):
    # a segment over the fuse bound keeps pass B (here split by column: 8 + 1 <= 16 workgroups)
    pass_b, fused, colsplit, grid = nat.long_window_shape_work(LIST, SEG_COLS, FLAT, 3, SPLIT_MAX, True)
    assert fused == [(0 << 20) | 2]
    assert pass_b == [e for c in range(NCHUNKS) for e in _split(1, c, 2)]
    assert colsplit is True and grid == 8
    # at this window a segment has 4 chunks, the product's bound: every segment is fused
    pass_b, fused, colsplit, grid = nat.long_window_shape_work(LIST, SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, True)
    assert (pass_b, fused, colsplit, grid) == ([], LIST, False, 0)


def test_shape_fuse_off_is_column_split(nat):
    pass_b, fused, colsplit, grid = nat.long_window_shape_work(LIST, SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, False)
    assert fused == []
    assert pass_b == _split(0, 2, 2) + [e for c in range(NCHUNKS) for e in _split(1, c, 2)]
    assert colsplit is True and grid == 10


def test_shape_split_only_when_it_fits(nat):
    # more column entries than the bound, or than the flat grid (the list's staging size): as listed
    assert nat.long_window_shape_work(LIST, SEG_COLS, FLAT, FUSE_CHUNKS, 9, False) == (LIST, [], False, 5)
    wide = [(0 << 20) | 2] + [(1 << 20) | c for c in range(NCHUNKS)]  # a 13-wide ring: 8 + 4 x 5 > 8
    assert nat.long_window_shape_work(wide, [8, 5], 8, FUSE_CHUNKS, SPLIT_MAX, False) == (wide, [], False, 5)


def test_shape_empty_list(nat):
    # fuse off: the grid's first workgroup must still copy the brackets - entry 0 (segment 0,
    # chunk 0), one workgroup per column of the segment
    assert nat.long_window_shape_work([], [1], NCHUNKS, FUSE_CHUNKS, SPLIT_MAX, False) == ([0], [], True, 1)
    assert nat.long_window_shape_work([], [8, 5], 8, FUSE_CHUNKS, SPLIT_MAX, False) == (_split(0, 0, 8), [], True, 8)
    assert nat.long_window_shape_work([], [8, 8, 8], 12, FUSE_CHUNKS, 4, False) == ([0], [], False, 1)
    # fuse on: lw_ingest copies them, no pass B at all
    assert nat.long_window_shape_work([], SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, True) == ([], [], False, 0)


def test_shape_full_list_is_the_flat_grid(nat):
    full = [(g << 20) | c for g in range(len(SEG_COLS)) for c in range(NCHUNKS)]
    for fuse in (False, True):
        assert nat.long_window_shape_work(full, SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, fuse) == ([], [], False, FLAT)
    assert nat.long_window_shape_work(full[:-1], SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, False)[3] == FLAT - 1


def test_bad_inputs_are_errors(nat):
    with pytest.raises(ValueError):
        nat.long_window_work_list(W, [(4, ROWS, NCHUNKS, 130)], [100], [1, 1, 1], [0, 0, 0, 0])  # a flag short
    with pytest.raises(ValueError):
        nat.long_window_work_list(W, [(13, ROWS, NCHUNKS, 130)], [100], [1] * 13, [0] * 13)  # one head for two segments
    with pytest.raises(ValueError):
        nat.long_window_shape_work([(4 << 20) | 1], SEG_COLS, FLAT, FUSE_CHUNKS, SPLIT_MAX, False)  # no segment 4
