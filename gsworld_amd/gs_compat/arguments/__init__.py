"""``arguments`` of the 3DGS python layer.  GSWorld imports only the ``PipelineParams`` name as a type annotation
(/root/reference/gsworld/mani_skill/utils/wrappers/gs_world_wrapper.py:13,37) and builds its own parameter groups
(/root/reference/gsworld/utils/gs_utils.py:22-106); the four pipeline flags below are the rasterizer's inputs."""


class GroupParams:
    pass


class PipelineParams:
    def __init__(self, parser=None, sentinel=False):
        self.convert_SHs_python = False
        self.compute_cov3D_python = False
        self.debug = False
        self.antialiasing = False
        if parser is not None:
            group = parser.add_argument_group("Pipeline Parameters")
            for key in ("convert_SHs_python", "compute_cov3D_python", "debug", "antialiasing"):
                group.add_argument("--" + key, default=False, action="store_true")

    def extract(self, args):
        group = GroupParams()
        for key in ("convert_SHs_python", "compute_cov3D_python", "debug", "antialiasing"):
            setattr(group, key, getattr(args, key, False))
        return group


class ParamGroup:
    """Upstream's argument group: every attribute the subclass set before calling this becomes ``--name`` with its value
    as the default and its type as the parser's; a leading underscore also gives the one-letter flag (``_source_path`` ->
    ``--source_path`` / ``-s``); a bool is a ``store_true`` switch.  ``fill_none``: every default is None (a parser whose
    unset values must not override a stored ``cfg_args``)."""

    def __init__(self, parser, name: str, fill_none: bool = False):
        group = parser.add_argument_group(name)
        for key, value in vars(self).items():
            flags = ["--" + key.lstrip("_")] if not key.startswith("_") else ["--" + key[1:], "-" + key[1:2]]
            default = None if fill_none else value
            if isinstance(value, bool):
                group.add_argument(*flags, default=default, action="store_true")
            else:
                group.add_argument(*flags, default=default, type=type(value))

    def extract(self, args):
        group = GroupParams()
        mine = vars(self)
        for key, value in vars(args).items():
            if key in mine or "_" + key in mine:
                setattr(group, key, value)
        return group


class ModelParams(ParamGroup):
    def __init__(self, parser, sentinel=False):
        self.sh_degree = 3
        self._source_path = ""
        self._model_path = ""
        self._images = "images"
        self._depths = ""
        self._resolution = -1
        self._white_background = False
        self.train_test_exp = False
        self.data_device = "cuda"
        self.eval = False
        super().__init__(parser, "Loading Parameters", sentinel)

    def extract(self, args):
        import os

        g = super().extract(args)
        g.source_path = os.path.abspath(g.source_path)
        return g


class OptimizationParams(ParamGroup):
    def __init__(self, parser):
        self.iterations = 30_000
        self.position_lr_init = 0.00016
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.feature_lr = 0.0025
        self.opacity_lr = 0.025
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.exposure_lr_init = 0.01
        self.exposure_lr_final = 0.001
        self.exposure_lr_delay_steps = 0
        self.exposure_lr_delay_mult = 0.0
        self.percent_dense = 0.01
        self.lambda_dssim = 0.2
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.depth_l1_weight_init = 1.0
        self.depth_l1_weight_final = 0.01
        self.random_background = False
        self.optimizer_type = "default"
        super().__init__(parser, "Optimization Parameters")


def get_combined_args(parser, argv=None):
    """The command line merged over the ``cfg_args`` file (``str(Namespace(...))``) the trainer left in ``--model_path``: a
    command-line value that is not None wins."""
    import os
    import sys
    from argparse import Namespace

    args_cmdline = parser.parse_args(sys.argv[1:] if argv is None else argv)
    stored = Namespace()
    try:
        path = os.path.join(args_cmdline.model_path, "cfg_args")
        print("Looking for config file in", path)
        with open(path) as f:
            print(f"Config file found: {path}")
            stored = eval(f.read(), {"Namespace": Namespace, "__builtins__": {}})  # noqa: S307
    except (TypeError, FileNotFoundError):
        print("Config file not found")
    merged = dict(vars(stored))
    merged.update({k: v for k, v in vars(args_cmdline).items() if v is not None})
    return Namespace(**merged)
