"""Hand-written grid cases of the frame composer, shared by the CPU tests (against frames_truth) and the GPU tests (against the
kernel): B = 3 images of 1 x 1 pixels, one or two panels, make_grid(padding=2) written out cell by cell. torchvision is not a
dependency, so these arrays ARE the pin of the layout: each entry is 0 (padding / empty cell) or the 1-based number of the image
whose pixel sits there (two panels: 10 * image + panel)."""
import numpy as np

# image k, panel p -> its RGB bytes; every byte b enters as float32(b) / 255, which the RGB rule returns exactly
COLOURS = {1: (10, 20, 30), 2: (40, 50, 60), 3: (70, 80, 90), 11: (10, 20, 30), 12: (11, 21, 31), 21: (40, 50, 60), 22: (41, 51, 61),
           31: (70, 80, 90), 32: (71, 81, 91)}

ONE_PANEL_NROW1 = [          # nrow = int(sqrt(3)) = 1: a column of three cells, frame 11 x 5
    [0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 1, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 2, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 3, 0, 0],
    [0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0]]

ONE_PANEL_NROW2 = [          # two columns, the fourth cell has no image, frame 8 x 8
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 1, 0, 0, 2, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 3, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0]]

ONE_PANEL_NROW5 = [          # nrow above B: xmaps = B, one row, frame 5 x 11
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]

TWO_PANELS_NROW2 = [         # strips of two pixels, frame 8 x 10
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 11, 12, 0, 0, 21, 22, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 31, 32, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]


def _expected(layout):
    table = np.zeros((100, 3), dtype=np.uint8)
    for k, c in COLOURS.items():
        table[k] = c
    return table[np.array(layout)][None]                       # [1, Hg, Wg, 3]


def _panel(codes):
    """[B, 3, 1, 1] float32 (a static panel) whose image k has the colour of COLOURS[codes[k]]."""
    return (np.array([COLOURS[c] for c in codes], dtype=np.float32) / np.float32(255)).reshape(len(codes), 3, 1, 1)


def hand_grid_cases():
    """[(name, panels as (array, kind, range_index), nrow, expected uint8 [1, Hg, Wg, 3])]"""
    one = [(_panel([1, 2, 3]), "rgb", None)]
    two = [(_panel([11, 21, 31]), "rgb", None), (_panel([12, 22, 32]), "rgb", None)]
    return [("one_panel_nrow_default", one, None, _expected(ONE_PANEL_NROW1)),
            ("one_panel_nrow2", one, 2, _expected(ONE_PANEL_NROW2)),
            ("one_panel_nrow5", one, 5, _expected(ONE_PANEL_NROW5)),
            ("two_panels_nrow2", two, 2, _expected(TWO_PANELS_NROW2))]
