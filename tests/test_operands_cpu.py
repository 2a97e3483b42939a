"""scrabble_gan_amd/operands.py alone, on CPU tensors: fp32 owners with bf16 / uint8 stand-ins for the copies.  The registry is
bookkeeping over storage pointers, offsets and sizes, so nothing here launches a kernel or needs the library."""
import ast

import pytest
import torch

from scrabble_gan_amd import operands


@pytest.fixture
def reg():
    return operands.Registry()


def f32(*shape):
    return torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float32).reshape(shape)


def u8(t):
    return torch.zeros(t.shape, dtype=torch.uint8)


def test_module_needs_only_torch():
    with open(operands.__file__) as f:
        tree = ast.parse(f.read())
    mods = {n.module if isinstance(n, ast.ImportFrom) else a.name
            for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
    assert mods == {"__future__", "dataclasses", "typing", "torch"}, mods


def test_slices_read_the_twin(reg):
    x = f32(4, 2, 3, 8)
    twin = x.to(torch.bfloat16)
    reg.put_bf16(x, twin)
    got = reg.get_bf16(x[1:3])
    assert got.shape == (2, 2, 3, 8) and got.dtype == torch.bfloat16
    assert got.data_ptr() == twin.data_ptr() + 2 * 48 and torch.equal(got, twin.view(-1)[48:144].view(2, 2, 3, 8))
    assert torch.equal(reg.get_bf16(x), twin)
    assert reg.get_bf16(f32(4, 2, 3, 8)) is None


def test_slices_register_nothing(reg):
    x = f32(4, 2, 3, 8)
    part = x[1:3]                       # offset 48
    head = x[:2]                        # offset 0, but half the storage
    for t in (part, head):
        reg.put_bf16(t, t.to(torch.bfloat16))
        reg.put_amax(t, torch.zeros(2), None)
    assert reg.count() == 0 and reg.find(x) is None
    assert reg.get_bf16(x) is None and reg.get_amax(x) is None and reg.storage_amax(part) is None


def test_amax_matching(reg):
    x, y = f32(4, 2, 3, 8), f32(4, 2, 3, 8)
    sp, sq = torch.ones(4), torch.ones(4)
    pair_x, pair_y = torch.zeros(2), torch.zeros(2)
    reg.put_amax(x, pair_x, sp)
    reg.put_amax(y, pair_y, None)
    assert reg.get_amax(x) is pair_x                                    # element 0 serves whatever the scale
    assert reg.get_amax(x, sp, need_scaled=True) is pair_x
    assert reg.get_amax(x, sq, need_scaled=True) is None
    assert reg.get_amax(x, None, need_scaled=True) is None
    assert reg.get_amax(y, None, need_scaled=True) is pair_y
    assert reg.get_amax(y, sp, need_scaled=True) is None
    for t in (x[1:3], x[:2]):
        assert reg.get_amax(t) is None and reg.get_amax(t, sp, need_scaled=True) is None
    assert reg.storage_amax(x[1:3]) is pair_x                           # (the one reader that lets a slice share it)


def test_copies_are_keyed_per_slice(reg):
    x = f32(4, 2, 3, 8)
    views = (x, x[1:3], x[:2])
    made = {}
    for relu in (False, True):
        for k, v in enumerate(views):
            assert reg.get_fp8(v, relu) is None
            made[relu, k] = reg.put_fp8(v, relu, u8(v), torch.zeros(1))
    assert len({id(e) for e in made.values()}) == 6
    for (relu, k), e in made.items():
        assert reg.get_fp8(views[k], relu) is e and e.data.shape == views[k].shape
    s1, s2 = torch.ones(4), torch.ones(4)
    b1 = reg.put_grad_bf16(x, s1, x.to(torch.bfloat16), None)
    b2 = reg.put_grad_bf16(x, s2, x.to(torch.bfloat16), torch.zeros(8))
    b0 = reg.put_grad_bf16(x, None, x.to(torch.bfloat16), None)
    assert reg.get_grad_bf16(x, s1) is b1 and reg.get_grad_bf16(x, s2) is b2 and reg.get_grad_bf16(x, None) is b0
    assert b1.colsum is None and b2.colsum is not None and reg.get_grad_bf16(x[1:3], s1) is None
    g1 = reg.put_grad_fp8(x, s1, u8(x), torch.zeros(1), None, torch.zeros(2))
    g2 = reg.put_grad_fp8(x, s2, u8(x), torch.zeros(1), None, torch.zeros(2))
    assert reg.get_grad_fp8(x, s1) is g1 and reg.get_grad_fp8(x, s2) is g2 and reg.get_grad_fp8(x, None) is None
    a1 = reg.put_amax2(x[1:3], s1, torch.zeros(2))
    assert reg.get_amax2(x[1:3], s1) is a1 and reg.get_amax2(x[1:3], s2) is None and reg.get_amax2(x, s1) is None
    assert reg.get_grad_bf16(x, s1) is b1                               # the families do not shadow one another


def _fill(reg, t, scale):
    reg.mark_ghost(t)
    reg.put_bf16(t, t.to(torch.bfloat16))
    reg.put_amax(t, torch.zeros(2), scale)
    reg.put_fp8(t[1:], True, u8(t[1:]), torch.zeros(1))
    reg.put_grad_bf16(t, scale, t.to(torch.bfloat16), None)
    reg.put_grad_fp8(t, scale, u8(t), torch.zeros(1), None, torch.zeros(2))
    reg.put_amax2(t[:1], scale, torch.zeros(2))
    reg.keep(t, True, 2, torch.zeros(16 * 128 * 8), 128, 7)


def test_touch_is_scoped_to_one_storage(reg):
    x, y, s = f32(2, 2, 4, 8), f32(2, 2, 4, 8), torch.ones(2)
    reg.keeping = True
    _fill(reg, x, s)
    _fill(reg, y, s)
    assert reg.count() == 14 and len(reg.ghosts) == 2 and reg.kept_count() == 2
    reg.touch(None)
    assert reg.count() == 14
    reg.touch(x[1:])                                                    # any view of the storage names it
    assert reg.find(x) is None and not reg.is_ghost(x) and len(reg.ghosts) == 1
    assert reg.get_bf16(x) is None and reg.get_amax(x) is None and reg.get_fp8(x[1:], True) is None
    assert reg.get_grad_bf16(x, s) is None and reg.get_grad_fp8(x, s) is None and reg.get_amax2(x[:1], s) is None
    assert reg.kept(x, True, 2) is None
    assert reg.count() == 7 and reg.is_ghost(y) and reg.kept_count() == 1
    assert reg.get_bf16(y) is not None and reg.get_amax(y, s, need_scaled=True) is not None and reg.get_fp8(y[1:], True) is not None
    assert reg.get_grad_bf16(y, s) is not None and reg.get_grad_fp8(y, s) is not None and reg.get_amax2(y[:1], s) is not None
    assert reg.kept(y, True, 2) is not None


def test_count_moves_by_one_per_stored_copy(reg):
    x, s = f32(2, 2, 4, 8), torch.ones(2)
    steps = [lambda: reg.put_bf16(x, x.to(torch.bfloat16)),
             lambda: reg.put_fp8(x, False, u8(x), torch.zeros(1)),
             lambda: reg.put_fp8(x[1:], False, u8(x[1:]), torch.zeros(1)),
             lambda: reg.put_grad_bf16(x, s, x.to(torch.bfloat16), None),
             lambda: reg.put_grad_fp8(x, s, u8(x), torch.zeros(1), None, torch.zeros(2)),
             lambda: reg.put_amax(x, torch.zeros(2), s),
             lambda: reg.put_amax2(x, None, torch.zeros(2)),
             lambda: reg.mark_ghost(x)]
    for k, put in enumerate(steps):
        assert reg.count() == k
        put()
        assert reg.count() == k + 1
        put()                                                           # the same copy again replaces, it does not add
        assert reg.count() == k + 1
    assert len(reg.ghosts) == 1
    reg.clear()
    assert reg.count() == 0 and not reg.ghosts and reg.find(x) is None


def test_kept_winograd_transform(reg):
    B, H, W, K, tile = 5, 4, 8, 16, 2
    x = f32(B, H, W, K)
    V = torch.zeros(16 * 128 * K)
    reg.keep(x, True, tile, V, 128, 7)
    for b0, b1 in ((0, B), (2, B), (0, 2), (3, 4)):
        e, row = reg.kept(x[b0:b1], True, tile)
        assert e.V is V and e.plane_rows == 128 and e.stream == 7
        assert row == b0 * (H // tile) * (W // tile)
    assert reg.kept(x, False, tile) is None                             # another operand ReLU
    assert reg.kept(x, True, 4) is None                                 # another tile size
    assert reg.kept(x.view(B, W, H, K), True, tile) is None             # another spatial shape
    assert reg.kept(x.view(-1)[K:K + 2 * H * W * K].view(2, H, W, K), True, tile) is None   # not on a sample boundary
    assert reg.kept(f32(B, H, W, K), True, tile) is None
    reg.end_step()
    assert reg.kept(x, True, tile) is None and reg.kept_count() == 0 and not reg.keeping


def test_steps_clear_what_they_should(reg):
    x = f32(2, 2, 4, 8)
    reg.new_step(True)
    assert reg.keeping
    _fill(reg, x, None)
    slot = reg.amax_slot(3, x.device)
    assert slot.shape == (2,) and reg.amax_slot(3, x.device).data_ptr() == slot.data_ptr() + 8      # one pool per stream handle ...
    assert reg.amax_slot(4, x.device).untyped_storage().data_ptr() != slot.untyped_storage().data_ptr()
    reg.end_step()                                                      # releases the kept transforms alone
    assert reg.count() == 7 and reg.kept_count() == 0
    assert reg.amax_slot(3, x.device).data_ptr() == slot.data_ptr() + 16
    reg.new_step(False)
    assert reg.count() == 0 and not reg.ghosts and not reg.keeping
    fresh = reg.amax_slot(3, x.device)                                  # ... handed out anew, zeroed, every step
    assert fresh.untyped_storage().data_ptr() != slot.untyped_storage().data_ptr() and not fresh.any()


def test_the_cap_empties_everything(reg):
    owners = [torch.zeros(8) for _ in range(operands.MAX_RECORDS + 1)]
    for t in owners:
        reg.mark_ghost(t)
        reg.put_bf16(t, t.to(torch.bfloat16))
    assert reg.count() == 2 * len(owners) and len(reg.ghosts) == len(owners)
    last = torch.zeros(8)
    reg.put_bf16(last, last.to(torch.bfloat16))                         # one record over the cap: all the others go, ghost marks included
    assert reg.count() == 1 and not reg.ghosts and reg.get_bf16(last) is not None
    assert not any(reg.is_ghost(t) for t in owners) and all(reg.get_bf16(t) is None for t in owners)


class _AtAddress:
    """Stands in for a [B] scale tensor that the allocator placed at a given address."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def test_amax_entry_keeps_its_scale_alive(reg):
    """The amax pair is matched by the ADDRESS of its scale, so the entry must own the scale: once freed, its address could be handed
    to another [B] tensor with other factors, and element 1 of the pair would answer for them."""
    import gc
    import weakref
    x, pair = f32(4, 2, 3, 8), torch.zeros(2)
    s1 = torch.ones(4)
    old, alive = s1.data_ptr(), weakref.ref(s1)
    before = reg.count()
    reg.put_amax(x, pair, s1)
    assert reg.count() == before + 1                                    # (the kept scale is no copy of its own)
    del s1
    gc.collect()
    assert alive() is not None and alive().data_ptr() == old, "the amax entry let go of its scale: its address can be recycled"
    assert reg.find(x).amax.scale is alive()
    later = [torch.full((4,), 8.0) for _ in range(64)]                  # same size: what the allocator would hand the freed block to
    assert all(t.data_ptr() != old for t in later)
    assert reg.get_amax(x, _AtAddress(old), need_scaled=True) is pair   # whoever is at that address IS the kept scale ...
    assert torch.equal(alive(), torch.ones(4))                          # ... and still holds the factors the pair was taken with
    assert reg.get_amax(x, later[0], need_scaled=True) is None
    reg.touch(x)                                                        # the record goes, and the scale with it
    gc.collect()
    assert alive() is None and reg.get_amax(x, _AtAddress(old), need_scaled=True) is None
    s2 = torch.ones(4)                                                  # the stand-alone pair is keyed the same way and keeps its scale too
    alive2 = weakref.ref(s2)
    reg.put_amax2(x, s2, pair)
    assert reg.count() == 1
    del s2
    gc.collect()
    assert alive2() is not None and reg.get_amax2(x, alive2()) is pair
    reg.touch(x)
    gc.collect()
    assert alive2() is None


def test_amax_without_a_scale_keeps_nothing(reg):
    x, pair = f32(4, 2, 3, 8), torch.zeros(2)
    reg.put_amax(x, pair, None)
    a = reg.find(x).amax
    assert a.scale is None and a.scale_ptr == 0 and reg.count() == 1
    assert reg.get_amax(x, None, need_scaled=True) is pair and reg.get_amax(x, _AtAddress(0), need_scaled=True) is pair


def test_drop_copies_keeps_the_ghost_marks(reg):
    x, y, s = f32(2, 2, 4, 8), f32(2, 2, 4, 8), torch.ones(2)
    _fill(reg, x, s)                                                    # a ghost with every kind of copy
    reg.put_bf16(y, y.to(torch.bfloat16))
    reg.put_fp8(y, False, u8(y), torch.zeros(1))
    reg.drop_copies()
    assert reg.count() == 1 and reg.is_ghost(x) and reg.find(x).count() == 0 and reg.find(x).owner is x
    assert reg.find(y) is None and reg.get_bf16(x) is None and reg.storage_amax(x) is None
    reg.touch(x)
    assert reg.count() == 0 and not reg.ghosts
