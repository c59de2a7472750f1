"""openpose/util.py: `handDetect`, `padRightDownCorner`, `npmax` and `transfer` as the reference computes them; the drawing functions
return the canvas unchanged and say so once on stderr (drawing is out of scope)."""
import numpy as np

from bodyfitting_amd import openpose as _op
from bodyfitting_amd import openpose_hand as _oh


def padRightDownCorner(img, stride, padValue):
    """pad the bottom and right to multiples of stride with padValue -> (img_padded, [up, left, down, right])"""
    h, w = img.shape[0], img.shape[1]
    pad = [0, 0, 0 if h % stride == 0 else stride - (h % stride), 0 if w % stride == 0 else stride - (w % stride)]
    out = np.full((h + pad[2], w + pad[3]) + tuple(img.shape[2:]), padValue, dtype=img.dtype)
    out[:h, :w] = img
    return out, pad


def transfer(model, model_weights):
    """the state dict of `model`'s keys with their first component (model0., model1_0., ...) dropped, looked up in model_weights"""
    return {name: model_weights[".".join(name.split(".")[1:])] for name in model.state_dict().keys()}


def handDetect(candidate, subset, oriImg):
    """[[x, y, w, is_left]] hand boxes per person of subset (left first), as util.handDetect computes them"""
    H, W = oriImg.shape[0:2]
    return _oh.hand_detect(candidate, subset, H, W)


def npmax(array):
    """(row, column) of the first occurrence of the maximum"""
    return _oh.npmax(np.asarray(array))


def draw_bodypose(canvas, candidate, subset):
    _op.warn_drawing("util.draw_bodypose")
    return canvas


def draw_handpose(canvas, all_hand_peaks, show_number=False):
    _op.warn_drawing("util.draw_handpose")
    return canvas


def draw_handpose_by_opencv(canvas, peaks, show_number=False):
    _op.warn_drawing("util.draw_handpose_by_opencv")
    return canvas
