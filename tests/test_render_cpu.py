"""The render stage without a GPU: tests/render_witness.py -- the numpy restatement of include/mscnn_hip.h's comment on
mscnn_render_detections_u8 that the GPU tests hold the kernel to, byte for byte -- against expected arrays written out by hand here,
the glyph table against the library's (mscnn_render_glyph_rows needs the built library and no device), and the ctypes structs
against the headers' sizeof."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_witness as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = (200, 100, 50)


def picture(rows, on, off):
    """[h, w, 3] from strings: '#' = on, anything else = off."""
    return np.array([[on if ch == "#" else off for ch in r] for r in rows], np.uint8)


def one(frame, rows, p, ids=None):
    return rw.render([frame], [[np.array(rows, np.float64).reshape(-1, 5)]], p, None if ids is None else [[np.array(ids)]])[0]


def test_one_box_on_an_8_x_10_frame():
    frame = np.full((8, 10, 3), 10, np.uint8)
    got = one(frame, [[2, 1, 5, 4, 0.9]], rw.params(thickness=1, label="none", colors=[COL]))
    want = picture(["..........",
                    "..#####...",
                    "..#...#...",
                    "..#...#...",
                    "..#####...",
                    "..........",
                    "..........",
                    ".........."], COL, (10, 10, 10))
    assert np.array_equal(got, want)
    # the footprint rounds: x = 1.5 -> L = 2, x + w = 6.49 -> R = 5
    got = one(frame, [[1.5, 0.6, 4.99, 4.3, 0.9]], rw.params(thickness=1, label="none", colors=[COL]))
    want = picture(["..........",
                    "..####....",
                    "..#..#....",
                    "..#..#....",
                    "..####....",
                    "..........",
                    "..........",
                    ".........."], COL, (10, 10, 10))
    assert np.array_equal(got, want)


def test_blend_rounds_at_alphas_0_77_and_256():
    assert rw.blend(10, 200, 77) == 67          # (10 * 179 + 200 * 77 + 128) >> 8 = 17318 >> 8
    assert rw.blend(255, 0, 77) == 178          # (255 * 179 + 128) >> 8 = 45773 >> 8
    assert rw.blend(0, 255, 77) == 77           # (255 * 77 + 128) >> 8 = 19763 >> 8
    frame = np.zeros((2, 3, 3), np.uint8)
    frame[...] = (10, 255, 0)
    for a, want in ((0, (10, 255, 0)), (77, (67, 178, 77)), (256, (200, 0, 255))):
        got = one(frame, [[1, 0, 1, 1, 0.9]], rw.params(thickness=0, fill_alpha=a, label="none", colors=[(200, 0, 255)]))
        assert tuple(got[0, 1]) == want, (a, got[0, 1])
        got[0, 1] = frame[0, 1]
        assert np.array_equal(got, frame)
        got = one(frame, [[1, 0, 1, 1, 0.9]], rw.params(thickness=1, outline_alpha=a, label="none", colors=[(200, 0, 255)]))
        assert tuple(got[0, 1]) == want, (a, got[0, 1])
    # fill first, then the outline over it
    got = one(frame, [[1, 0, 1, 1, 0.9]], rw.params(thickness=1, outline_alpha=77, fill_alpha=77, label="none", colors=[(200, 0, 255)]))
    assert tuple(got[0, 1]) == (rw.blend(67, 200, 77), rw.blend(178, 0, 77), rw.blend(77, 255, 77)) == (107, 124, 131)


def test_the_best_row_is_painted_last_and_a_later_slot_over_an_earlier_one():
    frame = np.zeros((4, 6, 3), np.uint8)
    red, green, blue = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    p = rw.params(thickness=64, label="none", color_by="id", colors=[blue, red, green])
    # one slot: row 0 (id 1, red) and row 1 (id 2, green) share columns 2 .. 3
    got = one(frame, [[0, 0, 4, 2, 0.9], [2, 0, 4, 2, 0.8]], p, ids=[1, 2])
    want = np.zeros((4, 6, 3), np.uint8)
    want[0:2, 0:4] = red
    want[0:2, 4:6] = green
    assert np.array_equal(got, want)
    # an id of 0 falls back to the slot's colour; two slots: slot 1 lies over slot 0
    segs = [[np.array([[0, 0, 4, 2, 0.9]]), np.array([[2, 0, 4, 2, 0.5]])]]
    got = rw.render([frame], segs, rw.params(thickness=64, label="none", color_by="id", colors=[blue, red]), [[np.array([0]), np.array([0])]])[0]
    want = np.zeros((4, 6, 3), np.uint8)
    want[0:2, 0:2] = blue
    want[0:2, 2:6] = red
    assert np.array_equal(got, want)
    # below the threshold: not drawn; a NaN score: not drawn
    got = one(frame, [[0, 0, 4, 2, 0.29], [0, 0, 4, 2, float("nan")]], rw.params(label="none"))
    assert np.array_equal(got, frame)


# "0.50" in 6 x 8 cells, the 5 x 7 glyph in a cell's columns 1 .. 5 and rows 1 .. 7, drawn here by hand
LABEL_050 = ["".join(cells) for cells in [
    ("......", "......", "......", "......"),
    ("..###.", "......", ".#####", "..###."),
    (".#...#", "......", ".#....", ".#...#"),
    (".#..##", "......", ".####.", ".#..##"),
    (".#.#.#", "......", ".....#", ".#.#.#"),
    (".##..#", "......", ".....#", ".##..#"),
    (".#...#", "...##.", ".#...#", ".#...#"),
    ("..###.", "...##.", "..###.", "..###."),
]]


def test_the_label_0_50_glyph_for_glyph():
    assert all(len(r) == 24 for r in LABEL_050)
    frame = np.full((20, 40, 3), 7, np.uint8)
    p = rw.params(thickness=0, label="score", colors=[COL])      # 299 * 200 + 587 * 100 + 114 * 50 = 124200 < 128000: white ink
    got = one(frame, [[5, 10, 30, 6, 0.5]], p)
    want = frame.copy()
    want[2:10, 5:29] = picture(LABEL_050, (255, 255, 255), COL)      # bottom row at T - 1 = 9, left column at L = 5
    assert np.array_equal(got, want)
    bright = (250, 250, 0)      # 299 * 250 + 587 * 250 = 221500 >= 128000: black ink
    got = one(frame, [[5, 10, 30, 6, 0.5]], rw.params(thickness=0, label="score", colors=[bright]))
    want = frame.copy()
    want[2:10, 5:29] = picture(LABEL_050, (0, 0, 0), bright)
    assert np.array_equal(got, want)


def test_every_label_placement_rule():
    p = rw.params(thickness=0, label="score", colors=[COL])
    lab = picture(LABEL_050, (255, 255, 255), COL)
    frame = np.full((20, 40, 3), 7, np.uint8)
    # its top row would be above the frame (T = 7 < 8): inside the box, top row at T
    got = one(frame, [[5, 7, 30, 10, 0.5]], p)
    want = frame.copy()
    want[7:15, 5:29] = lab
    assert np.array_equal(got, want)
    # past the right edge (L = 30, 30 + 24 > 40): shifted left to end at the edge
    got = one(frame, [[30, 10, 8, 6, 0.5]], p)
    want = frame.copy()
    want[2:10, 16:40] = lab
    assert np.array_equal(got, want)
    # a frame narrower than the label: not below column 0, clipped on the right
    narrow = np.full((20, 15, 3), 7, np.uint8)
    got = one(narrow, [[3, 10, 8, 6, 0.5]], p)
    want = narrow.copy()
    want[2:10, 0:15] = lab[:, :15]
    assert np.array_equal(got, want)
    # a box that starts left of the frame keeps its label at L: clipped on the left
    got = one(frame, [[-4, 10, 20, 6, 0.5]], p)
    want = frame.copy()
    want[2:10, 0:20] = lab[:, 4:]
    assert np.array_equal(got, want)
    # magnified twice: every label pixel is a 2 x 2 square
    big = np.full((40, 60, 3), 7, np.uint8)
    got = one(big, [[4, 20, 30, 6, 0.5]], rw.params(thickness=0, label="score", label_scale=2, colors=[COL]))
    want = big.copy()
    want[4:20, 4:52] = lab.repeat(2, axis=0).repeat(2, axis=1)
    assert np.array_equal(got, want)


def test_label_texts():
    assert rw.label_text(0.5, 0, 1) == "0.50" and rw.label_text(0.994, 0, 1) == "0.99" and rw.label_text(0.995, 0, 1) == "1.00"
    assert rw.label_text(1.7, 0, 1) == "1.00" and rw.label_text(-0.2, 0, 1) == "0.00" and rw.label_text(0.004, 0, 1) == "0.00"
    assert rw.label_text(0.5, 12, 2) == "12" and rw.label_text(0.5, 0, 2) == ""
    assert rw.label_text(0.25, 907, 3) == "907 0.25" and rw.label_text(0.25, 0, 3) == "0.25"
    assert rw.label_text(0.5, 2147483647, 3) == "2147483647 0.50"      # 15 characters: the longest a label gets


def test_a_mosaic_on_a_gradient_frame():
    frame = np.zeros((4, 6, 3), np.uint8)
    for y in range(4):
        for x in range(6):
            frame[y, x] = (10 * y + x, 0, 100)
    got = one(frame, [[1, 0, 4, 4, 0.9]], rw.params(thickness=0, label="none", pixelate=2))
    want = frame.copy()
    want[0:2, 1:3, 0] = 7       # (1 + 2 + 11 + 12 + 2) / 4
    want[0:2, 3:5, 0] = 9       # (3 + 4 + 13 + 14 + 2) / 4
    want[2:4, 1:3, 0] = 27      # (21 + 22 + 31 + 32 + 2) / 4
    want[2:4, 3:5, 0] = 29      # (23 + 24 + 33 + 34 + 2) / 4
    assert np.array_equal(got, want)
    # blocks of 3 anchored at (L, T) = (1, 0) and clipped to the box: columns {1, 2, 3} and {4}, rows {0, 1, 2} and {3}
    got = one(frame, [[1, 0, 4, 4, 0.9]], rw.params(thickness=0, label="none", pixelate=3))
    want = frame.copy()
    want[0:3, 1:4, 0] = 12      # (1 + 2 + 3 + 11 + 12 + 13 + 21 + 22 + 23 + 4) / 9 = 112 / 9
    want[0:3, 4, 0] = 14        # (4 + 14 + 24 + 1) / 3
    want[3, 1:4, 0] = 32        # (31 + 32 + 33 + 1) / 3
    want[3, 4, 0] = 34
    assert np.array_equal(got, want)
    # the mosaic discards what an earlier row painted there, and the later row's outline lies over it
    p = rw.params(thickness=1, label="none", pixelate=2, colors=[COL])
    got = one(frame, [[1, 0, 2, 2, 0.9], [0, 0, 6, 4, 0.5]], p)      # row 1 is painted first, row 0 over it
    first = one(frame, [[1, 0, 2, 2, 0.9]], p)
    assert np.array_equal(got[0:2, 1:3], first[0:2, 1:3]) and tuple(got[0, 1]) == COL
    assert tuple(got[0, 0]) == COL and tuple(got[1, 3]) == (8, 0, 100)      # row 1's block of columns {2, 3}: (2 + 3 + 12 + 13 + 2) / 4


def test_a_box_wholly_outside_the_frame_leaves_it_unchanged():
    frame = np.arange(8 * 10 * 3, dtype=np.uint8).reshape(8, 10, 3)
    p = rw.params(thickness=2, fill_alpha=100, label="score", pixelate=2)
    for row in ([10, 2, 5, 4, 0.9], [-9, 2, 8.4, 4, 0.9], [2, 8, 5, 4, 0.9], [2, -6, 5, 5.4, 0.9], [40, 30, 5, 4, 0.9]):
        assert np.array_equal(one(frame, [row], p), frame), row
    # rows without a footprint
    for row in ([2, 2, 0, 4, 0.9], [2, 2, 4, -1, 0.9], [2, 2, 0.4, 4, 0.9], [float("inf"), 2, 4, 4, 0.9], [2, 2, 4, float("nan"), 0.9],
                [2, 2, 2.0 ** 31, 4, 0.9], [-2.0 ** 30 + 8, 2, 2.0 ** 30 + 1, 4, 0.9], [2, 2, 4, 4, float("inf")]):
        assert np.array_equal(one(frame, [row], p), frame), row
    assert not np.array_equal(one(frame, [[-2.0 ** 30 + 8, 2, 2.0 ** 30, 4, 0.9]], p), frame)      # at the bound: drawn, R = 7


def test_the_glyph_table_equals_the_librarys():
    from mscnn_amd import hipapi
    for ch, rows in rw.GLYPHS.items():
        assert hipapi.render_glyph_rows(ch) == tuple(rows), ch
        assert all(0 <= r < 32 for r in rows)
    assert sorted(rw.GLYPHS) == sorted("0123456789. ")
    assert len({rw.GLYPHS[ch] for ch in "0123456789."}) == 11, "two characters share a bitmap"
    with pytest.raises(hipapi.MscnnError, match="render_glyph_rows: character 65 is none of"):
        hipapi.render_glyph_rows("A")


def sizeof_in_header(header, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stdint.h>\n#include "%s"\nint main(void) { printf("%%d %%d\\n", (int)sizeof(mscnn_render_params), '
                   '(int)offsetof(mscnn_render_params, colors)); return 0; }\n' % header)
    exe = tmp_path / "size"
    lang = ["-x", "c++"] if cc.endswith("hipcc") else []
    r = subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), *lang, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


@pytest.mark.parametrize("header", ["mscnn_hip.h", "mscnn_net.h"])
def test_the_ctypes_structs_have_the_headers_size(header, tmp_path):
    from mscnn_amd import hipapi, net
    size, colors_at = sizeof_in_header(header, tmp_path)
    assert size == 136 and colors_at == 40
    for S in (hipapi.RenderParams, net.RenderParams):
        assert C.sizeof(S) == size and S.colors.offset == colors_at
    p = hipapi.render_params([(1, 2, 3), (4, 5, 6)], show_thr=0.25, label="both", color_by="id", pixelate=8)
    assert (p.show_thr, p.label, p.color_by, p.pixelate, p.num_colors) == (0.25, 3, 1, 8, 2) and tuple(p.colors[1]) == (4, 5, 6)
    assert rw.LABELS == hipapi.RENDER_LABELS == net.RENDER_LABELS and rw.COLOR_BY == hipapi.RENDER_COLOR_BY == net.RENDER_COLOR_BY
    assert [tuple(c) for c in net.RENDER_PALETTE] == rw.PALETTE


def test_the_example_frame_for_a_persons_eye_is_a_rendered_frame():
    """tests/golden/render/render_example.png (tools/bench_render.py --example-out on an MI355X: the 16 best boxes of a synthetic kitti_car
    forward, label both, colour by track id, the lower-scored half pixelated): nobody can judge the look of the glyphs or the palette
    from a test, so this file is kept for a person to open.  Held here: it decodes to the frame's size, stays under the limit for a
    committed file, and opaque outlines and labels in every colour of the default palette are in it."""
    from PIL import Image
    path = os.path.join(ROOT, "tests", "golden", "render", "render_example.png")
    assert os.path.getsize(path) < (1 << 20)
    img = np.asarray(Image.open(path).convert("RGB"))
    assert img.shape == (375, 1242, 3)
    for col in rw.PALETTE:
        assert int((img == np.array(col, np.uint8)).all(axis=2).sum()) >= 500, col
