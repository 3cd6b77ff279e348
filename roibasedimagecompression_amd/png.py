"""python -m roibasedimagecompression_amd.png IN.png OUT.png --colours N [--refine R] [--dither S | --pattern S] [--exact]

A PNG file to a quantised PNG file on the device: ImageEncoder.quantize(IN, N, png_path=OUT) reads IN with container.read_png and
writes OUT with container.write_png; the host only reads and writes the files' bytes.  Prints the stats as one JSON line."""
import argparse
import json
import sys


def parser():
    p = argparse.ArgumentParser(prog="python -m roibasedimagecompression_amd.png", description="quantise a PNG file to a PNG file of N colours on the device")
    p.add_argument("src", metavar="IN.png")
    p.add_argument("dst", metavar="OUT.png")
    p.add_argument("--colours", type=int, required=True, metavar="N", help="at most N palette rows (a palette PNG up to 256, truecolour above)")
    p.add_argument("--refine", type=int, default=0, metavar="R", help="Lloyd iterations over the built palette (0..64)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--dither", type=int, default=None, metavar="S", help="error diffusion of strength S (0..256)")
    g.add_argument("--pattern", type=int, default=None, metavar="S", help="pattern dithering of strength S (0..256)")
    p.add_argument("--exact", action="store_true", help="IDAT through the level-9 encoder: the file is a function of the input alone")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    from .image import ImageEncoder
    res = ImageEncoder().quantize(args.src, args.colours, refine=args.refine, dither=args.dither, pattern=args.pattern, exact=args.exact, png_path=args.dst)
    print(json.dumps(res["stats"], sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
