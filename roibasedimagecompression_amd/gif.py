"""python -m roibasedimagecompression_amd.gif IN1.png IN2.png ... OUT.gif --colours N [--delay CS] [--loop N] [--no-delta] [--refine R]
       [--pattern S --pattern-size N]
   python -m roibasedimagecompression_amd.gif IN.gif OUT.gif --colours N [the same options]

PNG files of one size to an animated GIF on the device: every IN is read with container.read_png, ImageEncoder.animate builds one palette
for all frames, maps them and writes OUT; the host only reads and writes the files' bytes.  A lone input whose name ends in .gif is an
animation itself: it is read with container.read_gif (container.reduce_gif) and keeps its own delays and loop count unless --delay or
--loop say otherwise.  Prints the stats as one JSON line."""
import argparse
import json
import sys


def parser():
    p = argparse.ArgumentParser(prog="python -m roibasedimagecompression_amd.gif",
                                description="PNG files, or one animated GIF, to an animated GIF of N colours on the device")
    p.add_argument("files", metavar="FILE", nargs="+", help="IN1.png IN2.png ... OUT.gif, or IN.gif OUT.gif")
    p.add_argument("--colours", type=int, required=True, metavar="N", help="at most N palette rows (1..256; 255 with delta)")
    p.add_argument("--delay", type=int, default=None, metavar="CS", help="centiseconds a frame is shown (0..65535; default 4, a GIF input: its own)")
    p.add_argument("--loop", type=int, default=None, metavar="N", help="how often the animation repeats (0: for ever; default 0, a GIF input: its own)")
    p.add_argument("--no-delta", action="store_true", help="write every frame in full instead of marking unchanged pixels transparent")
    p.add_argument("--refine", type=int, default=0, metavar="R", help="Lloyd iterations over the shared palette (0..64)")
    p.add_argument("--pattern", type=int, default=None, metavar="S", help="pattern dithering of strength S (0..256): frame-stable")
    p.add_argument("--pattern-size", type=int, default=4, metavar="N", help="side of the threshold matrix (2, 4 or 8)")
    return p


def gif_input(files):
    """the inputs (the output's name taken off) are one animated GIF"""
    return len(files) == 1 and files[0].lower().endswith(".gif")


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if len(args.files) < 2:
        p.error("at least one input file and the output file are expected")
    from . import container
    from .image import ImageEncoder
    enc = ImageEncoder()
    if gif_input(args.files[:-1]):
        frames = args.files[0]
    else:
        frames = [container.read_png(name, enc.rh)["image"] for name in args.files[:-1]]
    res = enc.animate(frames, args.colours, gif_path=args.files[-1], delay=args.delay, loop=args.loop, delta=not args.no_delta, refine=args.refine,
                      pattern=args.pattern, pattern_size=args.pattern_size)
    print(json.dumps(res["stats"], sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
