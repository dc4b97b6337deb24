"""eval_instances.py with --matcher host (no GPU): both prediction formats against tests/ap_ref64.py, the refusals by name, and a
gloo world-2 run whose result file is the single process's, byte for byte."""
import json
import math
import os

import numpy as np
import pytest

import ap_ref64 as R
import ap_scenes as S


def flags(gt_dir, pred_dir, out, *more):
    return ['--gt-folder', gt_dir, '--prediction-folder', pred_dir, '--matcher', 'host', '--result-file', str(out), '--num_workers', '2'] + list(more)


def run(argv):
    from panoptic_forecasting_amd import eval_instances
    return eval_instances.run(eval_instances.parse_args(argv))


def check_against(res, ref, n_images, n_predictions, min_region):
    clean = lambda x: None if math.isnan(x) else x
    assert res['averages']['allAp'] == clean(ref['allAp']) and res['averages']['allAp50%'] == clean(ref['allAp50%'])
    for name in R.CLASS_NAMES:
        assert res['averages']['classes'][name] == {'ap': clean(ref['classes'][name]['ap']), 'ap50%': clean(ref['classes'][name]['ap50%'])}, name
    assert res['thresholds'] == np.arange(0.5, 1.0, 0.05).tolist() and res['min_region'] == min_region
    assert res['images'] == n_images and res['predictions']['total'] == n_predictions


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('ap_tree'))
    masks, image, labels, scores, gt, notes = S.hand_scene()
    gt_dir, pred_dir, stems = S.write_tree(root, masks, image, labels, scores, gt)
    return {'root': root, 'gt': gt_dir, 'pred': pred_dir, 'stems': stems, 'scene': (masks, image, labels, scores, gt)}


@pytest.mark.parametrize('min_region,more', [(100, ()), (3, ('--max-masks-per-call', '4', '--batch_size', '2')), (1, ('--batch_size', '1'))])
def test_cityscapes_format_equals_the_restatement(tree, tmp_path, min_region, more):
    masks, image, labels, scores, gt = tree['scene']
    out = tmp_path / 'r.json'
    res = run(flags(tree['gt'], tree['pred'], out, '--min-region', str(min_region), *more))
    with open(out) as f:
        assert json.load(f) == res
    check_against(res, R.evaluate(S.per_image(masks, image, labels, scores, gt), min_region), 3, len(masks), min_region)
    assert res['predictions'] == {'total': len(masks), 'counted': len(masks) - 3, 'empty': 1, 'not_an_instance_class': 2}
    assert res['averages']['classes']['train']['ap'] == 0.0 and res['averages']['classes']['person']['ap'] is None
    assert 0 < res['averages']['allAp'] < 1


def test_the_result_does_not_depend_on_batching_or_the_mask_limit(tree, tmp_path):
    files = []
    for k, more in enumerate([(), ('--max-masks-per-call', '1'), ('--max-masks-per-call', '5', '--batch_size', '3'), ('--batch_size', '1')]):
        out = tmp_path / ('r%d.json' % k)
        run(flags(tree['gt'], tree['pred'], out, '--min-region', '3', *more))
        files.append(out.read_bytes())
    assert all(f == files[0] for f in files)


def test_panoptic_format_equals_the_restatement(tree, tmp_path):
    """Thing segments of a labelId * 1000 + id map, each an instance of confidence 1.0."""
    rng = np.random.default_rng(4)
    gt, _, _, _, _ = S.random_scene((3, 40, 60), 21, 1)
    seg = np.where(rng.random(gt.shape) < 0.15, 7, gt)              # the ground truth with holes ...
    seg[:, :3] = 26000 + 77                                            # ... and a car nobody asked for
    seg[seg == 0] = 8
    seg = np.where((seg < 1000) & (seg > 33), 7, seg)
    root = str(tmp_path)
    blank = np.zeros((0, 40, 60), np.uint8)
    gt_dir, _, stems = S.write_tree(root, blank, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), gt)
    pan_dir = S.write_panoptic(root, seg, stems)
    out = tmp_path / 'pan.json'
    res = run(flags(gt_dir, pan_dir, out, '--prediction-format', 'panoptic', '--min-region', '3', '--max-masks-per-call', '3'))
    images, total = [], 0
    for i in range(3):
        values = [v for v in np.unique(seg[i]).tolist() if v >= 1000 and v // 1000 in R.INSTANCE_LABELS]
        total += len(values)
        images.append((np.stack([seg[i] == v for v in values]) if values else blank, [v // 1000 for v in values], [1.0] * len(values), gt[i]))
    assert total >= 6
    check_against(res, R.evaluate(images, 3), 3, total, 3)
    assert res['averages']['allAp'] is not None and res['averages']['allAp'] > 0


def test_refusals_name_what_is_wrong(tree, tmp_path):
    import shutil
    from panoptic_forecasting_amd.eval_common import EvalError
    from panoptic_forecasting_amd import lib
    masks, image, labels, scores, gt = tree['scene']
    out = tmp_path / 'r.json'
    stem = tree['stems'][1]

    def copy():
        dst = str(tmp_path / ('pred%d' % len(os.listdir(str(tmp_path)))))
        shutil.copytree(tree['pred'], dst)
        return dst

    pred = copy()
    os.remove(os.path.join(pred, stem + '.txt'))
    with pytest.raises(EvalError, match='no prediction %s.txt for ground-truth image' % stem):
        run(flags(tree['gt'], pred, out))
    pred = copy()
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('../outside.png 26 0.5\n')
    with pytest.raises(EvalError, match='leaves the prediction folder'):
        run(flags(tree['gt'], pred, out))
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('%s 26 0.5\n' % os.path.join(pred, 'masks', os.listdir(os.path.join(pred, 'masks'))[0]))
    with pytest.raises(EvalError, match='leaves the prediction folder'):
        run(flags(tree['gt'], pred, out))
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('masks/missing.png 26 0.5\n')
    with pytest.raises(EvalError, match='no mask file masks/missing.png'):
        run(flags(tree['gt'], pred, out))
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('masks/x.png 26\n')
    with pytest.raises(EvalError, match='line 1: expected "mask.png labelID confidence"'):
        run(flags(tree['gt'], pred, out))
    from PIL import Image
    Image.fromarray(np.ones((4, 6), np.uint8)).save(os.path.join(pred, 'masks', 'small.png'))
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('masks/small.png 26 0.5\n')
    with pytest.raises(EvalError, match='ground truth is 40x60, mask .*small.png 4x6'):
        run(flags(tree['gt'], pred, out))
    with open(os.path.join(pred, stem + '.txt'), 'w') as f:
        f.write('masks/small.png 34 0.5\n')
    with pytest.raises(EvalError, match='labelID 34 is outside'):
        run(flags(tree['gt'], pred, out))
    with pytest.raises(EvalError, match='no ground truth'):
        run(flags(pred, pred, out))
    with pytest.raises(EvalError, match='no prediction .*_pred_panoptic.png'):
        run(flags(tree['gt'], tree['pred'], out, '--prediction-format', 'panoptic'))
    import torch
    if not torch.cuda.is_available():
        argv = flags(tree['gt'], tree['pred'], out)
        argv[argv.index('host')] = 'device'
        with pytest.raises(EvalError, match='--matcher device needs a GPU'):
            run(argv)
    with pytest.raises(lib.PfError, match='runs on the GPU'):
        from panoptic_forecasting_amd import instance_ap
        instance_ap.InstanceAP(device='cpu')


def test_an_empty_txt_means_no_predictions(tree, tmp_path):
    masks, image, labels, scores, gt = tree['scene']
    import shutil
    pred = str(tmp_path / 'pred')
    shutil.copytree(tree['pred'], pred)
    open(os.path.join(pred, tree['stems'][0] + '.txt'), 'w').close()
    res = run(flags(tree['gt'], pred, tmp_path / 'r.json', '--min-region', '3'))
    keep = image != 0
    check_against(res, R.evaluate(S.per_image(masks[keep], image[keep], labels[keep], scores[keep], gt), 3), 3, int(keep.sum()), 3)


def test_two_gloo_ranks_write_the_single_process_file(tree, tmp_path):
    import ap_eval_worker
    masks, image, labels, scores, gt = tree['scene']
    one, two = tmp_path / 'one.json', tmp_path / 'two.json'
    more = ('--min-region', '3', '--max-masks-per-call', '4', '--batch_size', '2')
    run(flags(tree['gt'], tree['pred'], one, *more))
    ap_eval_worker.spawn_two(flags(tree['gt'], tree['pred'], two, *more))
    assert one.read_bytes() == two.read_bytes()
    with open(two) as f:
        check_against(json.load(f), R.evaluate(S.per_image(masks, image, labels, scores, gt), 3), 3, len(masks), 3)
