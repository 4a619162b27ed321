"""The reference's `gallery` command (main.py:98-139 category lists, :163-200 helpers, :203-278 the command): one image through
every species of a category, the outputs laid out as a labelled contact sheet (gallery_grid.build_labeled_grid).

Non-interactive: the image path and the category are arguments instead of InquirerPy prompts.

    python -m animal_vision_amd.gallery photo.jpg --category UV --output-dir out/"""
from __future__ import annotations

import argparse
import os
import sys
import warnings
from datetime import datetime
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .gallery_grid import build_labeled_grid

# main.py:98-139, literally (UV_NAMES carries the unique-UV species too, as the reference's list does)
NON_UV_NAMES = [
    "Cat", "Dog", "Sheep", "Pig", "Goat", "Cow", "Horse", "Rabbit", "Panda", "Squirrel",
    "Elephant", "Lion", "Wolf", "Fox", "Bear", "Raccoon", "Deer", "Kangaroo", "Tiger", "Rat",
]
UV_NAMES = [
    "HoneyBee", "ReinDeer", "RatUV", "GoldFish", "DamselFish", "Anableps (Four-eyed fish)", "Northern Anchovy Fish",
    "Guppy Fish", "Morpho Butterfly", "Heliconius Butterfly", "Pieris Butterfly",
    # Unique UV animals
    "Mantis Shrimp", "Kestrel", "Jumping Spider", "DragonFly", "HummingBird",
]
UNIQUE_UV_NAMES = ["Mantis Shrimp", "Kestrel", "Jumping Spider", "DragonFly", "HummingBird"]
CATEGORIES = {"Non-UV": NON_UV_NAMES, "UV": UV_NAMES, "Unique-UV": UNIQUE_UV_NAMES}

# utils.py:91-130 (animal_choices): display name -> class name in animals/
_CLASS_NAMES = {
    "Cat": "Cat", "Dog": "Dog", "Sheep": "Sheep", "Pig": "Pig", "Goat": "Goat", "Cow": "Cow", "Horse": "Horse", "Rabbit": "Rabbit",
    "Panda": "Panda", "Squirrel": "Squirrel", "Elephant": "Elephant", "Lion": "Lion", "Wolf": "Wolf", "Fox": "Fox", "Bear": "Bear",
    "Raccoon": "Raccoon", "Deer": "Deer", "Kangaroo": "Kangaroo", "Tiger": "Tiger", "Rat": "Rat",
    "HoneyBee": "HoneyBee", "ReinDeer": "Reindeer", "RatUV": "RatUV", "GoldFish": "Goldfish", "DamselFish": "Damselfish",
    "Anableps (Four-eyed fish)": "Anableps", "Northern Anchovy Fish": "Anchovy", "Guppy Fish": "Guppy", "Morpho Butterfly": "Morpho",
    "Heliconius Butterfly": "Heliconius", "Pieris Butterfly": "Pieris",
    "Mantis Shrimp": "MantisShrimp", "Kestrel": "Kestrel", "Jumping Spider": "JumpingSpider", "DragonFly": "Dragonfly",
    "HummingBird": "Hummingbird",
}


def species_class(name: str) -> type:
    """The class behind a display name of animal_choices."""
    from . import animals

    return getattr(animals, _CLASS_NAMES[name])


def names_for_category(category: str) -> List[str]:
    """_names_for_category, strict: anything but "Non-UV", "UV" or "Unique-UV" raises ValueError."""
    try:
        return CATEGORIES[category]
    except (KeyError, TypeError):
        raise ValueError(f"category must be one of {sorted(CATEGORIES)} (got {category!r})") from None


def ensure_rgb_uint8(img: np.ndarray) -> np.ndarray:
    """_ensure_rgb_uint8 (main.py:163-171): float -> clip to [0, 1], * 255 + 0.5, truncate; uint8 as is."""
    if img.dtype == np.uint8:
        return img
    if np.issubdtype(img.dtype, np.floating):
        return (np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    raise NotImplementedError(f"dtype {img.dtype}: uint8 and floating-point images are supported")


def _output_of(res) -> Optional[np.ndarray]:
    """_run_visualize_get_output's unpacking: (base, out) -> out, or base when out is None; a bare array as is."""
    if res is None:
        return None
    if isinstance(res, tuple) and len(res) == 2:
        base, out = res
        return out if out is not None else base
    return res


def gallery(image: np.ndarray, category: str, *, tile_height: int = 256,
            choices: Optional[Sequence[Tuple[str, object]]] = None) -> Optional[np.ndarray]:
    """Every species of `category` on `image` (RGB, uint8 or float in [0, 1]), as one labelled grid (RGB uint8), or None when no
    species produced an output.  `choices`: (display name, animal) pairs to run instead of the category's registry species.  A
    species that raises is skipped with a warning, as the reference skips it."""
    names = names_for_category(category)
    src = ensure_rgb_uint8(np.asarray(image))
    runs: List[Tuple[str, Callable[[], object]]]
    if choices is None:
        runs = [(n, (lambda n=n: species_class(n)())) for n in names]  # constructed when its turn comes, default arguments
    else:
        runs = [(n, (lambda a=a: a)) for n, a in choices]
    tiles = []
    for name, make in runs:
        try:
            out = _output_of(make().visualize(src))
        except Exception as e:  # noqa: BLE001 -- the reference's behaviour: warn and go on with the next species
            warnings.warn(f"gallery: {name} failed ({type(e).__name__}: {e}); skipped", RuntimeWarning, stacklevel=2)
            continue
        if out is None:
            warnings.warn(f"gallery: {name} returned no output; skipped", RuntimeWarning, stacklevel=2)
            continue
        tiles.append((name, ensure_rgb_uint8(np.asarray(out))))
    return build_labeled_grid(tiles, tile_height=tile_height, pad=8, bg=(20, 20, 20))


def output_name(category: str, when: Optional[datetime] = None) -> str:
    """main.py:270-271: gallery_{NonUV|UV|UniqueUV}_{YYYYmmdd_HHMMSS}.png."""
    ts = (when or datetime.now()).strftime("%Y%m%d_%H%M%S")
    return f"gallery_{category.replace('-', '').replace(' ', '')}_{ts}.png"


def main(argv: Optional[Sequence[str]] = None) -> int:
    """`python -m main gallery` without the prompts: read the image (Pillow, as ImageRenderer), build the sheet, save it as
    output_dir/gallery_<category>_<timestamp>.png and print that path."""
    ap = argparse.ArgumentParser(prog="gallery", description="Labelled grid of every species of a category on one image.")
    ap.add_argument("input", help="image file (png / jpg)")
    ap.add_argument("--category", default="Non-UV", choices=list(CATEGORIES))
    ap.add_argument("--tile-height", type=int, default=256)
    ap.add_argument("--output-dir", default=".")
    args = ap.parse_args(argv)

    from .renderers.image import ImageRenderer

    src = ImageRenderer(args.input).get_image()
    grid = gallery(src, args.category, tile_height=args.tile_height)
    if grid is None:
        print("Nothing to render for this category.")
        return 1
    os.makedirs(args.output_dir, exist_ok=True)
    out_path = os.path.join(args.output_dir, output_name(args.category))
    from PIL import Image

    Image.fromarray(grid).save(out_path)
    print(f"Saved gallery: {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
