"""The odd, unaligned image sizes the training tapes are checked at (tests/test_grad_shapes_gpu.py,
tests/test_train_shapes_gpu.py), beside the exact-halving 64 x 96 / 96 x 128 of the older tape
tests.  tests/test_grad_shapes_refs.py proves on the CPU that they are what they claim and that the
float64 references hold there.

    A  52 x 76, B 2:  C2..C5 = 13 x 19, 7 x 10, 4 x 5, 2 x 3   (the FPN branch's second pyramid)
    B  72 x 100, B 3: C2..C5 = 18 x 25, 9 x 13, 5 x 7, 3 x 4   (117 + 35 + 12 = 164 encoder tokens)
    C  61 x 87, B 2:  C2..C5 = 16 x 22, 8 x 11, 4 x 6, 2 x 3   (the train pipeline's own odd batch
                                                                tensor; half-size masks 30 x 43)

`pyramid` is the size arithmetic of the tapes themselves (`BackboneGrad.forward`: a stride-2 step
maps n to (n - 1) // 2 + 1), restated; plain Python, shares no code with the package."""
from collections import namedtuple

Shape = namedtuple("Shape", "name H W B counts")

A = Shape("A", 52, 76, 2, (3, 5))
B = Shape("B", 72, 100, 3, (3, 5, 2))
C = Shape("C", 61, 87, 2, (3, 5))
OLD = Shape("64x96", 64, 96, 2, (3, 5))             # what the tape tests ran before: every step exact
TAPE_SHAPES = [A, B]
IMAGE_SHAPES = [A, B, C]


def step(n):
    """One stride-2 step with a 3-wide kernel and padding 1 (or 1-wide, padding 0): ceil(n / 2)."""
    return (n - 1) // 2 + 1


def pyramid(H, W):
    """(h, w) of C2, C3, C4, C5 for an image of H x W: stem convolution, max pool, three stages."""
    h, w = step(step(H)), step(step(W))
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = step(h), step(w)
    return out


def floor_pyramid(H, W):
    """What a tape that floored at every stride-2 step behind C2 would believe."""
    h, w = pyramid(H, W)[0]
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def key_counts(s):
    """Keys per masked-decoder level (coarsest first: C5, C4, C3), as `plan.N` lists them."""
    return [h * w for h, w in reversed(pyramid(s.H, s.W)[1:])]


def encoder_tokens(s):
    return sum(key_counts(s))


def gt_mask_size(s):
    """The ground-truth masks the segmentation losses take: half the image, floored."""
    return s.H // 2, s.W // 2


def metas(s):
    return [dict(img_shape=(s.H, s.W, 3), scale_factor=[1.5] * 4)] * s.B
