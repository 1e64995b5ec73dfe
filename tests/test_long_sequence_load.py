"""CPU tier: the load-time sequence-length cap.  Every supported head size takes up to 1025 tokens per sequence (32 x 32 patches + the
class token: ViT-L/14 at 448 px, ViT-B/16 at 512 px); sequences past the whole-row attention kernel (592 keys at d_head 64, 288 at the
other head sizes) run the streaming kernel of k_attn_long.hip.  No GPU needed: clip_model_load returns a host-only context here."""
import os

import pytest

from oracle import fixtures

TINY = fixtures.CONFIGS["tiny"]


def _vision(S, P, h, nh):
    return dict(v=dict(S=S, P=P, h=h, L=1, nh=nh, ff=64, proj=32), t=TINY["t"])


def _load(L, path):
    ctx = L.clip_model_load(os.fsencode(path), 0)
    if ctx:
        L.clip_free(ctx)
    return bool(ctx)


@pytest.mark.parametrize("name,cfg", [
    ("h14_378", _vision(378, 14, 320, 4)),      # T = 27*27 + 1 = 730, d_head 80 (ViT-H/14 at 378 px)
    ("l14_448", _vision(448, 14, 128, 2)),      # T = 32*32 + 1 = 1025, d_head 64 (ViT-L/14 at 448 px)
    ("b16_512", _vision(512, 16, 128, 2)),      # T = 1025, d_head 64 (ViT-B/16 at 512 px)
    ("big_g_336", _vision(336, 14, 832, 8)),    # T = 577, d_head 104 (ViT-bigG/14 at 336 px)
    ("g_448", _vision(448, 14, 704, 8)),        # T = 1025, d_head 88 (the loader wants hidden sizes that are multiples of 64)
])
def test_long_vision_towers_load(clip_lib, tmp_path, host_only_env, capfd, name, cfg):
    L = clip_lib.lib()
    path = str(tmp_path / (name + ".gguf"))
    fixtures.make_model(path, cfg, "f32", text=False, vision=True)
    assert _load(L, path), capfd.readouterr().err


def test_long_text_tower_loads_up_to_the_cap(clip_lib, tmp_path, host_only_env, capfd):
    L = clip_lib.lib()
    path = str(tmp_path / "t1025.gguf")
    fixtures.make_model(path, dict(v=TINY["v"], t=dict(TINY["t"], npos=1025)), "f32", text=True, vision=False)
    assert _load(L, path), capfd.readouterr().err


@pytest.mark.parametrize("tower", ["text", "vision"])
def test_sequences_past_1025_tokens_are_refused(clip_lib, tmp_path, host_only_env, capfd, tower):
    L = clip_lib.lib()
    path = str(tmp_path / (tower + ".gguf"))
    if tower == "text":      # 1026 context positions, d_head 32
        fixtures.make_model(path, dict(v=TINY["v"], t=dict(TINY["t"], npos=1026)), "f32", text=True, vision=False)
    else:                    # 33*33 + 1 = 1090 tokens, d_head 64
        fixtures.make_model(path, _vision(462, 14, 128, 2), "f32", text=False, vision=True)
    capfd.readouterr()
    assert not _load(L, path)
    err = capfd.readouterr().err
    assert "tokens per sequence" in err and "> 1025" in err, err
