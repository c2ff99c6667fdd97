"""vpt_scene_filter_volumes on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere: a resident
scene after filter_volumes(edit) against the host mirror (HostScene.filter_volume, held to float64 by tests/test_filter_host.py) and
against a fresh DeviceScene made from the filtered host scene.  The scene is 10_volgrid_synth's "messy": volume 0 (9 x 17 x 30, with NaN,
+-Inf and negative voxels, or replaced by a grid of the case's shape) is filtered, volume 1 lies directly behind it in the pool."""
import numpy as np
import pytest

from test_volgrid_host import load

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ops_of(vpt, names):
    make = {"noise": lambda: vpt.FilterOp.noise(0.75, (9.0, 7.5, 11.0), 0.55, 4, seed=11), "density": lambda: vpt.FilterOp.to_density(0.4),
            "remap": lambda: vpt.FilterOp.remap(-0.5, 2.0, 0.1, -1.0, 4.0), "noise1": lambda: vpt.FilterOp.noise(-0.3, 40.0, 0.9, 8, seed=0xffffffff),
            **{f"blur{r}": (lambda r=r: vpt.FilterOp.blur(0.8 * r, r)) for r in (1, 2, 3, 4)}}
    return [make[n]() for n in names.split()]


def pair(vpt, shape):
    """(a resident scene, the host scene it was made from): volume 0 the messy grid (shape None) or a random grid of `shape` = (w, h, d)"""
    host = load(vpt, "messy")
    if shape is not None:
        host.set_volume(0, np.random.default_rng(sum(shape)).normal(0, 1, shape[::-1]).astype(F), res=0.05)
        host.update_volumes()
    dev = vpt.DeviceScene(host, 0)
    vols = dev.get_volumes()[0]
    assert vols[1].offset == vols[0].offset + int(np.prod(list(vols[0].whd)))   # volume 1 directly behind volume 0
    return dev, host


def launches_of(ops):
    """one per run of pointwise ops, two per blur"""
    kinds = [op.type == 1 for op in ops]
    return 2 * sum(kinds) + sum(1 for i, b in enumerate(kinds) if not b and (i == 0 or kinds[i - 1]))


WHOLE, INNER = None, ((3, 1, 5), (5, 10, 2))
CASES = [   # (shape of volume 0 or None for the messy grid, region, ops)
    ((1, 1, 1), WHOLE, "noise density blur1"), ((1, 1, 1), WHOLE, "blur4 remap"), ((3, 5, 2), WHOLE, "blur4"), ((3, 5, 2), WHOLE, "remap blur2 noise1"),
    (None, WHOLE, "blur1"), (None, WHOLE, "blur4"), (None, WHOLE, "noise density"), (None, INNER, "blur4"), (None, INNER, "noise blur1 remap"),
    ((9, 17, 30), WHOLE, "noise density blur3 blur1"), ((9, 17, 30), INNER, "blur2 noise1"), ((9, 17, 30), ((0, 0, 29), (9, 17, 1)), "blur4 density"),
    ((20, 9, 9), WHOLE, "blur2"), ((20, 9, 9), ((1, 0, 2), (18, 9, 6)), "blur4 noise remap blur1"),
]


@pytest.mark.parametrize("shape,region,names", CASES, ids=[f"{s}-{'inner' if r else 'whole'}-{n.replace(' ', '_')}" for s, r, n in CASES])
def test_filter_equals_the_mirror_and_a_fresh_scene(vpt, shape, region, names):
    A, host = pair(vpt, shape)
    before, behind = host.volume(0)[0].copy(), bits(A.get_voxels(1)).copy()
    entry = host.filter_volume(0, ops_of(vpt, names), region=region)
    edit = host.update_filters()
    A.filter_volumes(edit)
    launches, sent, ms = A.update_stats()
    print(f"{shape} {region} {names}: {(launches, sent, ms)} (launches, bytes, device ms)", flush=True)
    assert (launches, sent) == (launches_of(entry.ops), vpt.FILTER_RECORD_BYTES * len(entry.ops)) and sent == edit.payload_bytes()
    got, want = bits(A.get_voxels(0)), bits(host.volume(0)[0])
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} voxels differ from the host mirror's"
    assert np.array_equal(bits(A.get_voxels(1)), behind), "the volume behind changed"
    lo, size = ((0, 0, 0), got.shape[::-1]) if region is None else region
    outside = np.ones(got.shape, bool)
    outside[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = False
    assert np.array_equal(got[outside], bits(before)[outside]) and not np.array_equal(got[~outside], bits(before)[~outside])
    B = vpt.DeviceScene(host, 0)
    assert np.array_equal(bits(B.get_voxels(0)), got) and np.array_equal(bits(B.get_voxels(1)), behind)


def test_an_op_list_equals_its_ops_one_edit_each_and_nothing_to_do_launches_nothing(vpt):
    A, host = pair(vpt, (20, 9, 9))
    entry = host.filter_volume(0, ops_of(vpt, "noise density blur2"), region=((1, 0, 2), (18, 9, 6)))
    A.filter_volumes(host.update_filters())
    assert A.update_stats()[:2] == (3, 3 * 48)
    B, _ = pair(vpt, (20, 9, 9))
    for op in entry.ops:
        B.filter_volumes(vpt.FilterEdit([vpt.FilterEntry(0, entry.region_lo, entry.region_whd, entry.origin, entry.step, [op])]))
    assert np.array_equal(bits(A.get_voxels(0)), bits(B.get_voxels(0)))
    idle = vpt.FilterEdit([vpt.FilterEntry(0, (1, 1, 1), (0, 3, 3), 0.0, 1.0, entry.ops), vpt.FilterEntry(1, (0, 0, 0), (2, 2, 2), 0.0, 1.0, [])])
    B.filter_volumes(idle)
    assert B.update_stats()[:2] == (0, 0) == (0, idle.payload_bytes()) and np.array_equal(bits(A.get_voxels(0)), bits(B.get_voxels(0)))


def render(vpt, host, dev):
    p = vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=4, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, 4)
    return st


def same_state(a, b):
    return a.samples == b.samples and np.array_equal(bits(a.image), bits(b.image)) and np.array_equal(a.hits, b.hits) and np.array_equal(a.rngs, b.rngs)


def test_volgrid_majorants_and_renders_follow_a_filter(vpt):
    A, host = pair(vpt, None)
    first = render(vpt, host, A)   # the brick tables exist before the edit: they have to be made anew
    builds = A.volgrid_stats()["table_builds"]
    host.filter_volume(0, ops_of(vpt, "remap blur2 noise"))
    A.filter_volumes(host.update_filters())
    got, want = A.volgrid_majorants(0), host.volgrid_majorants(0)
    assert np.array_equal(bits(got), bits(want)) and A.volgrid_stats()["table_builds"] == builds + 1
    after = render(vpt, host, A)
    assert same_state(after, render(vpt, host, vpt.DeviceScene(host, 0))) and not same_state(after, first)


def test_session_edit_filters_resets_and_a_refused_edit_leaves_it(vpt):
    host = load(vpt, "messy")
    s = vpt.RenderSession(vpt.DeviceScene(host, 0), vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=8, bounces=4))
    s.advance(2)
    host.filter_volume(0, ops_of(vpt, "remap blur1"))
    s.edit_filters(host.update_filters())
    assert s.samples == 0
    s.advance(2)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=8, bounces=4))
    fresh.advance(2)
    assert same_state(s.state(), fresh.state())
    for entries, named in (([vpt.FilterEntry(0, (8, 0, 0), (2, 1, 1), 0.0, 1.0, ops_of(vpt, "blur1"))], "entry 0: the region leaves the grid"),
                           ([vpt.FilterEntry(2, (0, 0, 0), (1, 1, 1), 0.0, 1.0, ops_of(vpt, "blur1"))], "entry 0: volume 2 out of range"),
                           ([vpt.FilterEntry(0, (0, 0, 0), (1, 1, 1), 0.0, 1.0, [vpt.FilterOp.remap(0, 1, 0, 0, 1)])], "op 0: divisor is 0")):
        with pytest.raises(vpt.VptError, match=named):
            s.edit_filters(vpt.FilterEdit(entries))
        assert s.samples == 2
    assert same_state(s.state(), fresh.state())
    s.close(), fresh.close()
