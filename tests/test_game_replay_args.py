"""CPU: the argument checks of alphazero.game_replay(..., init=...) that are made before any device is touched."""
import numpy as np
import pytest

import rule_positions as rp


@pytest.fixture(scope="module")
def az():
    import __graft_entry__ as g
    g.build()
    import alphazero
    return alphazero


def test_row_count_must_match_the_moves(az):
    img = az.Connect4GS(np.zeros((2, 6, 7), np.int8), 0, 0)._init
    assert len(img) == 89
    moves = -np.ones((3, 1), np.int32)
    with pytest.raises(RuntimeError, match="2 start positions for 3 move rows"):
        az.game_replay(az.Connect4GS, moves, init=[img, img])
    with pytest.raises(RuntimeError, match="4 start positions for 3 move rows"):
        az.game_replay(az.Connect4GS, moves, init=np.zeros((4, 89), np.uint8))
    with pytest.raises(RuntimeError, match=r"\[n, stride\]"):
        az.game_replay(az.Connect4GS, moves, init=np.zeros(3 * 89, np.uint8))


def test_connect4_stride_must_be_89(az):
    moves = -np.ones((2, 1), np.int32)
    for stride in (88, 90):
        with pytest.raises(RuntimeError, match="Connect4 images are 89 bytes"):
            az.game_replay(az.Connect4GS, moves, init=np.zeros((2, stride), np.uint8))
    with pytest.raises(RuntimeError, match="Connect4 images are 89 bytes"):
        az.game_replay(az.Connect4GS, moves, init=[b"\0" * 89, b"\0" * 90])       # padded to the longest: 90


@pytest.mark.parametrize("spec", rp.TAFL_SPECS, ids=lambda s: s.name)
def test_tafl_images_are_checked_on_the_host(az, spec):
    Game = getattr(az, spec.name)
    moves = -np.ones((2, 1), np.int32)
    img = Game._image(np.zeros((3, spec.N, spec.N), np.int8), 0, 5)
    assert len(img) == 3 * spec.N ** 2 + 10
    with pytest.raises(RuntimeError, match="a Tafl image is at least"):
        az.game_replay(Game, moves, init=[img[:-1], img[:-1]])
    lying = bytearray(img); lying[-4] = 1                                         # claims one repetition entry it does not bring
    with pytest.raises(RuntimeError, match="start position 1: repetition entry count mismatch"):
        az.game_replay(Game, moves, init=[img, bytes(lying)])
