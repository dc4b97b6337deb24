#!/usr/bin/env python
"""fg panoptic export driver with the reference's flags - drop-in for ``experiments/export_cityscapes_panoptic_results.py``.

    python -u panoptic-forecasting_amd/export_panoptic.py --config_file configs/fg/fg_val_mid.yaml \\
        --load_model pretrained_models/fg/fg_model.pt --export_name exported_panoptics_mid --working_dir experiments/pretrained_fg/ \\
        --extra_args data.background_dir experiments/pretrained_bg/exported_predictions_mid_trainids

i.e. the export command of ``scripts/fg/run_fg_eval_panoptic.sh:21-26`` with the python path changed.  Same flags
(``--export_name``, ``--no_convert`` + the base set of ``utils/config.py:34-45``), same output tree
(``<working_dir>/<export_name|exported_panoptics>_<split>/<same name>/{city}_{seq}_{target:06d}_pred_panoptic.png`` and
``<working_dir>/<...>_<split>/<...>_<split>.json``, ``:78-87,170-173``), same fill of missing frames (``:124-169``,
``panoptic.fill_missing_panoptic``).

The loop is serial: ``fg_dataset.NativeFGSceneDataset`` (host selection + one ``pf_fg_assemble`` launch per batch) ->
``build_model(params).predict_panoptic`` -> ``panoptic.export_panoptic`` (conversion and RGB encoding on the device).  No reference
code, pandas or h5py is needed where the ``.npz`` twins of the dataset's files exist (``fg_dataset.convert_to_npz``).
``--save_depth`` is accepted, as the reference parses it, and - as there - never read; ``--viz`` does not exist in this script.

One difference: without ``data.cityscapes_dir`` the reference returns before it writes the annotation file (``:126-128``); here the
pass over missing frames alone is skipped and the annotations of what was exported are written.
"""
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__ in (None, ''):                     # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(_HERE))
    import panoptic_forecasting_amd  # noqa: F401
    __package__ = 'panoptic_forecasting_amd'

from . import config as pfconfig   # noqa: E402
from . import fg_dataset           # noqa: E402
from . import panoptic             # noqa: E402
from .registry import build_model  # noqa: E402

EXTRA_FLAGS = (
    ('--save_depth', dict(action='store_true')),
    ('--export_name', {}),
    ('--no_convert', dict(action='store_true')),
)


def export_split(model, dataset, split, params):
    """export_results (:70-173) for one split; returns (result_dir, annotation file, number of annotations)."""
    if params.get('no_gpu'):
        raise SystemExit('export_panoptic: --no_gpu is not supported (the fg path has no CPU implementation)')
    no_convert = bool(params.get('no_convert'))
    print('NO CONVERT: ', no_convert)
    name = '%s_%s' % (params.get('export_name') or 'exported_panoptics', split)
    result_dir = os.path.join(params['working_dir'], name)
    os.makedirs(os.path.join(result_dir, name), exist_ok=True)
    annotations = []
    for batch in dataset.batches(int(params['training']['batch_size'])):
        with torch.no_grad():
            preds = model.predict_panoptic(batch['inputs'], batch['labels'])
        panoptic.export_panoptic(preds['seg'], batch['meta'], result_dir, name, no_convert=no_convert, annotations=annotations)
    cityscapes_dir = params['data'].get('cityscapes_dir')
    if cityscapes_dir is None:
        print('DID NOT RECEIVE CITYSCAPES DIR. SKIPPING.')
    else:
        print('CHECKING FOR MISSING FILES...')
        panoptic.fill_missing_panoptic(result_dir, name, os.path.join(cityscapes_dir, 'gtFine', dataset.split),
                                       background_dir=dataset.background_dir, annotations=annotations)
    print('NUM FINAL ANNOTATIONS: ', len(annotations))
    return result_dir, panoptic.write_annotations(annotations, result_dir, name), len(annotations)


def main(argv=None):
    params = pfconfig.load_config(EXTRA_FLAGS, argv)
    torch.manual_seed(params['seed'])
    data = fg_dataset.build_dataset(params, test=True)        # sets data.num_classes / odom_size / img_size, as the reference's does
    model = build_model(params)
    model.eval()
    out = {}
    for split, dataset in data.items():
        out[split] = export_split(model, dataset, split, params)
        dataset.close()
    return out


if __name__ == '__main__':
    main()
