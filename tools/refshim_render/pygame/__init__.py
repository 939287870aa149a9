"""numpy stand-in for the five pygame primitives the fork's colour-fallback
`_render_frame` uses (gradio-app/plantos_env_new.py:697-762), so that
tools/gen_golden_render.py can run the reference's own `env.render()` where pygame is
not installed.  `image.load` raises: the reference's `except:` then selects the
sprite-less path.

Everything specific to the environment (colours, layer order, ray march, end points,
truncations) stays the reference's code; only these primitives are this project's
definitions, chosen close to pygame's (DESIGN.md "Rendering": pixel parity with a real
pygame is not pinned for the line, the disc and the alpha blend):

  rectangle fill   the rectangle clipped to the surface
  alpha blit       per channel ((d << 8) + (s - d) * a + s) >> 8 (a = 0 keeps d)
  line             1-px integer Bresenham, both end points plotted, pixels off the
                   surface dropped (the unclipped line is walked)
  disc             pixels with dx*dx + dy*dy <= r*r
  array export     surfarray.array3d: [W, H, 3]
"""
import types

import numpy as np

SRCALPHA = 0x00010000
_init = False


def init():
    global _init
    _init = True


def get_init():
    return _init


def quit():  # noqa: A001
    global _init
    _init = False


class Rect:
    def __init__(self, x, y, w, h):
        self.x, self.y, self.w, self.h = int(x), int(y), int(w), int(h)


class Surface:
    def __init__(self, size, flags=0):
        w, h = int(size[0]), int(size[1])
        self.alpha = bool(flags & SRCALPHA)
        self.px = np.zeros((h, w, 4 if self.alpha else 3), np.uint8)  # [row, column, channel]

    def get_size(self):
        return self.px.shape[1], self.px.shape[0]

    def _color(self, color):
        c = [int(v) for v in color]
        if self.alpha:
            return c + [255] if len(c) == 3 else c
        return c[:3]

    def _plot(self, x, y, color):
        if 0 <= x < self.px.shape[1] and 0 <= y < self.px.shape[0]:
            self.px[y, x] = color

    def blit(self, src, dest):
        x0, y0 = (dest.x, dest.y) if isinstance(dest, Rect) else (int(dest[0]), int(dest[1]))
        h, w = src.px.shape[:2]
        if (x0, y0) != (0, 0) or (h, w) != self.px.shape[:2]:
            raise NotImplementedError("stand-in: whole-surface blit at (0, 0) only")
        if not src.alpha:
            self.px[..., :3] = src.px
            return
        d = self.px[..., :3].astype(np.int32)
        s = src.px[..., :3].astype(np.int32)
        a = src.px[..., 3:4].astype(np.int32)
        self.px[..., :3] = (((d << 8) + (s - d) * a + s) >> 8).astype(np.uint8)


def _rect(surface, color, rect, width=0):
    if width:
        raise NotImplementedError("stand-in: filled rectangles only")
    h, w = surface.px.shape[:2]
    x0, y0 = max(rect.x, 0), max(rect.y, 0)
    x1, y1 = min(rect.x + rect.w, w), min(rect.y + rect.h, h)
    if x0 < x1 and y0 < y1:
        surface.px[y0:y1, x0:x1] = surface._color(color)


def _line(surface, color, start, end, width=1):
    if width != 1:
        raise NotImplementedError("stand-in: 1-px lines only")
    c = surface._color(color)
    x, y = int(start[0]), int(start[1])
    x2, y2 = int(end[0]), int(end[1])
    dx, dy = abs(x2 - x), abs(y2 - y)
    sx = 1 if x < x2 else -1
    sy = 1 if y < y2 else -1
    err = int((dx if dx > dy else -dy) / 2)  # truncated toward zero
    while True:
        surface._plot(x, y, c)
        if x == x2 and y == y2:
            break
        e2 = err
        if e2 > -dx:
            err -= dy
            x += sx
        if e2 < dy:
            err += dx
            y += sy


def _circle(surface, color, center, radius, width=0):
    if width:
        raise NotImplementedError("stand-in: filled discs only")
    c = surface._color(color)
    cx, cy, r = int(center[0]), int(center[1]), int(radius)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy <= r * r:
                surface._plot(cx + dx, cy + dy, c)


def _load(path):
    raise FileNotFoundError("stand-in: no image loading (selects the reference's colour fallback)")


def _array3d(surface):
    return np.ascontiguousarray(np.transpose(surface.px[..., :3], (1, 0, 2)))


draw = types.SimpleNamespace(rect=_rect, line=_line, circle=_circle)
image = types.SimpleNamespace(load=_load)
surfarray = types.SimpleNamespace(array3d=_array3d)
