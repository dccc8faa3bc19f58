"""The binding's tile lists against the library's tile table (csrc/gemm_tiles.h, the one place a tile id is written in the
library): the ids the tuner tries per operand class, the tiles the grouped kernels are built for, the group size."""
import os
import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "fastspeech2_lightning_amd" / "csrc"
#: families that read bf16 operands from memory (fs2_family_stored in gemm_tiles.h); the others take fp32 operands
STORED = {"FS2_TF_B", "FS2_TF_BP", "FS2_TF_WS_K256", "FS2_TF_WS_K1024"}


def rows():
    text = (CSRC / "gemm_tiles.h").read_text()
    found = re.findall(r"^\s*\{\s*(\d+),\s*(FS2_TF_\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false)\s*\},", text, flags=re.M)
    assert len(found) == len({r[0] for r in found}) >= 26, "one row per tile id"
    return [(int(i), fam, int(bm), int(bn), int(depth), grouped == "true") for i, fam, bm, bn, depth, grouped in found]


def constant(name, text):
    return int(re.search(rf"\b{name} = (\d+)", text).group(1))


def test_binding_tile_lists_are_the_rows_of_the_tile_table():
    assert not os.environ.get("FS2_GEMM_EXCLUDE_TILES"), "run with FS2_GEMM_EXCLUDE_TILES unset"
    from fastspeech2_lightning_amd import hip
    table = rows()
    assert set(re.findall(r"FS2_TF_\w+", (CSRC / "gemm_tiles.h").read_text().split("struct Fs2Tile")[0])) == {r[1] for r in table}
    assert sorted(hip.GEMM_TILES_B) == sorted(r[0] for r in table if r[1] in STORED)
    assert sorted(hip.GEMM_TILES) == sorted(r[0] for r in table if r[1] not in STORED)
    assert sorted(r[0] for r in table) == list(range(1, 16)) + list(range(20, 27)) + list(range(30, 34))
    grouped = {0: sorted(r[0] for r in table if r[5] and r[1] not in STORED),
               4: sorted(r[0] for r in table if r[5] and r[1] in STORED)}
    assert {k: sorted(v) for k, v in hip.GROUP_TILES.items()} == grouped
    # the first tile of a class is the one fs2hip_gemm_grouped takes for tile 0
    text = (CSRC / "gemm_tiles.h").read_text()
    assert hip.GROUP_TILES[0][0] == constant("FS2_TILE_GROUP_DEFAULT", text)
    assert hip.GROUP_TILES[4][0] == constant("FS2_TILE_GROUP_DEFAULT_B", text)
    header = (REPO / "include" / "fs2hip.h").read_text()
    assert hip.GROUP_MAX == int(re.search(r"#define FS2_GEMM_GROUP_MAX (\d+)", header).group(1))
