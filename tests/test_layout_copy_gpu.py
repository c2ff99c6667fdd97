"""The plain copies between row-major pixels and tile-major slots (csrc/vpt_layout.hip), through the entry points that are nothing
else: vpt_state_upload, vpt_state_download, vpt_resolve_ids_device and vpt_resolve_sdf_ids_device.  No scene: layouts and buffers.
The expected arrays are numpy scatters and gathers through vpt.layout_pixel_index, which shares no code with the device, and the
comparison is of raw 32-bit words, exact.  Every word of every buffer is a running counter of its own range, so a wrong width,
stride or plane shows; every word the copy must leave alone holds a sentinel no counter reaches.
The layouts go past what the scene tests use: tiles other than 8x8 under the id gathers, frames smaller than a tile, and rank
counts that leave ranks without a pixel (13x21 in 32x16 tiles on 5 ranks: one tile).  The largest rank buffer has 4608 slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (7, 9), (8, 8), (13, 21), (70, 33)]
TILES = [(8, 8), (16, 8), (32, 16)]
RANKS = [1, 2, 3, 5]
SENTINEL = np.uint32(0xDEADBEEF)


def _layouts(vpt):
    for w, h in FRAMES:
        for tw, th in TILES:
            for n in RANKS:
                yield [vpt.VptLayout(w, h, tw, th, r, n) for r in range(n)]


def _counter(entries, words, base):
    """(entries, words) uint32, every word distinct and below the sentinel"""
    return (np.arange(entries * words, dtype=np.uint32) + np.uint32(base)).reshape(entries, words)


def _to_device(words):
    import torch
    return torch.from_numpy(words.view(np.int32).copy()).to(torch.device("cuda", 0))


def _words(tensor):
    return tensor.cpu().numpy().view(np.uint32)


def _host_state(vpt, w, h, image, hits, rng):
    """a PathtraceState over (pixels, words) uint32 arrays"""
    return vpt.PathtraceState(w, h, 0, image.view(np.float32).reshape(h, w, 4).copy(), hits.view(np.int32).reshape(h, w).copy(),
                              rng.view(np.uint64).reshape(h, w, 2).copy())


def _state_words(state):
    return [state.image.view(np.uint32).reshape(-1, 4), state.hits.view(np.uint32).reshape(-1, 1), state.rngs.view(np.uint32).reshape(-1, 4)]


def test_layouts_cover_every_pixel_once_and_leave_ranks_empty(vpt):
    """what the cases below rely on, on the host mirror alone"""
    empty = 0
    for ranks in _layouts(vpt):
        owned = [vpt.layout_pixel_index(lay) for lay in ranks]
        assert max(len(i) for i in owned) <= 4608
        every = np.concatenate([i[i >= 0] for i in owned])
        assert np.array_equal(np.sort(every), np.arange(ranks[0].width * ranks[0].height))
        empty += sum(1 for i in owned if not (i >= 0).any())
    assert empty > 0


def test_state_upload_writes_owned_slots_only(vpt):
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    for ranks in _layouts(vpt):
        w, h = ranks[0].width, ranks[0].height
        host = [_counter(w * h, 4, 0x10000000), _counter(w * h, 1, 0x20000000), _counter(w * h, 4, 0x30000000)]
        state = _host_state(vpt, w, h, *host)
        for lay in ranks:
            idx = vpt.layout_pixel_index(lay)
            own = idx >= 0
            tiles = [_to_device(np.full((len(idx), k), SENTINEL, np.uint32)) for k in (4, 1, 4)]
            vpt.state_upload(lay, state, *(t.data_ptr() for t in tiles))
            for got, src in zip(tiles, host):
                expect = np.full((len(idx), src.shape[1]), SENTINEL, np.uint32)
                expect[own] = src[idx[own]]
                assert np.array_equal(_words(got), expect), (w, h, lay.tile_w, lay.tile_h, lay.rank, lay.nranks)
        for got, src in zip(_state_words(state), host):   # the host arrays are read only
            assert np.array_equal(got, src)


def test_state_download_writes_owned_pixels_only(vpt):
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    for ranks in _layouts(vpt):
        w, h = ranks[0].width, ranks[0].height
        for lay in ranks:
            idx = vpt.layout_pixel_index(lay)
            own = idx >= 0
            src = [_counter(len(idx), 4, 0x10000000), _counter(len(idx), 1, 0x20000000), _counter(len(idx), 4, 0x30000000)]
            tiles = [_to_device(s) for s in src]
            state = _host_state(vpt, w, h, *(np.full((w * h, k), SENTINEL, np.uint32) for k in (4, 1, 4)))
            vpt.state_download(lay, *(t.data_ptr() for t in tiles), state)
            for got, s, t in zip(_state_words(state), src, tiles):
                expect = np.full((w * h, s.shape[1]), SENTINEL, np.uint32)
                expect[idx[own]] = s[own]
                assert np.array_equal(got, expect), (w, h, lay.tile_w, lay.tile_h, lay.rank, lay.nranks)
                assert np.array_equal(_words(t), s)   # the tiles are read only


@pytest.mark.parametrize("entry,words", [("resolve_ids_device", 3), ("resolve_sdf_ids_device", 4)])
@pytest.mark.parametrize("second", [False, True])
def test_id_gathers_write_every_pixel_from_its_slot(vpt, entry, words, second):
    """ids (8 bytes) alone, and with uvt (12 bytes) / hit (16 bytes), over the concatenated buffers of all ranks"""
    import torch
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    for ranks in _layouts(vpt):
        w, h, n = ranks[0].width, ranks[0].height, len(ranks)
        owned = [vpt.layout_pixel_index(lay) for lay in ranks]
        slots = len(owned[0])
        widths = (2, words) if second else (2,)
        src = [_counter(n * slots, k, 0x10000000 * (j + 1)) for j, k in enumerate(widths)]
        tiles = [_to_device(s) for s in src]
        rows = [_to_device(np.full((w * h, k), SENTINEL, np.uint32)) for k in widths]
        getattr(vpt, entry)(ranks[0], tiles[0].data_ptr(), tiles[1].data_ptr() if second else None, rows[0].data_ptr(),
                            rows[1].data_ptr() if second else None)
        torch.cuda.synchronize()
        for got, s, t in zip(rows, src, tiles):
            expect = np.full((w * h, s.shape[1]), SENTINEL, np.uint32)
            for r, idx in enumerate(owned):
                own = idx >= 0
                expect[idx[own]] = s[r * slots:(r + 1) * slots][own]
            assert not (expect == SENTINEL).any()   # every pixel has an owner: no sentinel is left in the rows
            assert np.array_equal(_words(got), expect), (w, h, ranks[0].tile_w, ranks[0].tile_h, n)
            assert np.array_equal(_words(t), s)
