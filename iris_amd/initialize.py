"""The initialisation stage (reference: initialize.py): the first estimate of the emitters' radiance under a default response model, with the material
network trained towards the segment means of the albedo prior.  It writes the `init.ckpt` that `extract_emitter_ldr --mode update` and
`train_brdf_crf --ckpt_path` read.

    python -m iris_amd.initialize --experiment_name EXP --dataset real DIR --ldr_img_dir ldr --voxel_path OUT/vslf.npz --emitter_path OUT/emitter.pth \
        --SPP 128 --spp 32 --crf_basis 3 --max_epochs 6 --checkpoint_path checkpoints --log_path logs

The stage is iris_amd.train_emitter.RadianceTrainer with mode='initialize'; what is built and what is not is said there.
"""
from . import train_emitter as _stage
from .utils.stage import exit_status


def parser():
    return _stage.parser("initialize", "the initialisation stage")


def cli_parser():
    """parser() and --validate (train_emitter.cli_parser): what main() parses"""
    return _stage.cli_parser("initialize", "the initialisation stage")


def main(argv=None):
    return _stage.run(cli_parser().parse_args(argv), "initialize", "initialize")


def cli(argv=None):
    return exit_status("initialize", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
