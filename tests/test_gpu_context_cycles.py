"""A context's resources go with it: eight cycles of create, resize, enable the AOVs, render, denoise, update the sample mask, read
back and close give the same bytes every time, for a plain context and for a group of two members on device 0.  Everything a context
holds is freed by its members' destructors (heatray_amd/csrc/hr_owned.h); a handle freed twice, or one freed while still in use,
shows here as a fault or as other bytes.  (Nothing is asserted about free device memory: that number belongs to everybody on the device.)

The frame is 40 x 24 with 32-pixel tiles: a partial tile on each axis."""
import pytest

from device_support import BOTH, render_passes, same
from heatray_amd import core, scenes

pytestmark = pytest.mark.gpu
CYCLES = 8


def cycle(create):
    sc = scenes.cornell_box(width=40, height=24, bounces=2)
    eng = create()
    sc.apply(eng)
    eng.resize(40, 24)
    eng.set_aovs(BOTH)
    render_passes(eng, sc, range(2))
    denoised = eng.denoise()
    eng.adaptive_update(install=True)
    frame = eng.readback()
    eng.close()
    assert frame.shape == (24, 40, 4) and (frame[..., 3] == 2).all()
    return frame, denoised


@pytest.mark.parametrize("create", [core.create_engine, lambda: core.create_group([0, 0])], ids=["plain", "group of 2"])
def test_every_cycle_of_a_contexts_life_gives_the_first_ones_bytes(create):
    first = cycle(create)
    for k in range(1, CYCLES):
        frame, denoised = cycle(create)
        same(frame, first[0], f"cycle {k}: frame")
        same(denoised, first[1], f"cycle {k}: denoised image")
