"""The HE2RNA baseline experiment -- counterpart of the ``__main__`` of the reference's ``src/he2rna.py`` (:323-436; same flags,
same outputs): a patient k-fold over the cohort; per fold an ``HE2RNA(layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100])`` is
trained with ``fit``, the test fold is predicted once before training (the ``random`` entry) and once after, and
``model_<fold>.pt`` (the whole module, what ``cli/visualize.py --model_type he2rna`` loads) and ``test_results.pkl`` (what
``cli/evaluate_model.py`` reads) are written under ``<destfolder>/<subfolder>/<exp_name>/``.

Beyond the reference's flags: ``--max_epochs`` / ``--patience`` (its ``fit`` defaults, 200 / 100), ``--dropout`` (the model's
default, 0.5) and ``--engine``: ``fused`` trains on He2rnaTrainStep (one C call per pass, validation score on the device),
``autograd`` on the torch optimiser loop.  fp32, one process."""
import argparse
import os
import pickle

import pandas as pd
import torch
from torch.utils.data import DataLoader

from ..data import CohortTable, ResidentLoader, SuperTileRNADataset, custom_collate_fn, filter_no_features, patient_kfold
from .common import seed_everything

LAYERS, KS = [256, 256], [1, 2, 5, 10, 20, 50, 100]


def build_parser():
    p = argparse.ArgumentParser(description='HE2RNA baseline: patient k-fold training and test predictions')
    p.add_argument('--path_csv', type=str, help='reference CSV: one row per slide with its rna_* expression columns')
    p.add_argument('--feature_path', type=str, default="features/", help='root of the per-slide feature stores (cluster_features)')
    p.add_argument('--checkpoint', type=str, help='a pickled HE2RNA (model_<fold>.pt) to start every fold from')
    p.add_argument('--change_num_genes', action="store_true", help='the checkpoint predicts another gene list: replace its head')
    p.add_argument('--num_genes', type=int, help='width of the checkpoint head (with --change_num_genes)')
    p.add_argument('--seed', type=int, default=99, help='seed of numpy, torch and the dropout stream')
    p.add_argument('--log', type=int, default=1, help='log to wandb when it is importable')
    p.add_argument('--k', type=int, default=5, help='folds of the patient k-fold')
    p.add_argument('--batch_size', type=int, default=16, help='slides per step')
    p.add_argument('--lr', type=float, default=1e-3, help='Adam step size')
    p.add_argument('--num_workers', type=int, default=0, help='accepted for compatibility; the loaders run in-process')
    p.add_argument('--tcga_projects', default=None, type=str, nargs='*', help='keep only the rows of these projects')
    p.add_argument('--exp_name', type=str, default="exp", help='last component of the output directory')
    p.add_argument('--subfolder', type=str, default="", help='middle component of the output directory')
    p.add_argument('--destfolder', type=str, default="", help='first component of the output directory')
    p.add_argument('--max_epochs', type=int, default=200, help='epochs per fold at most')
    p.add_argument('--patience', type=int, default=100, help='epochs without a better validation score before a fold stops')
    p.add_argument('--engine', choices=['fused', 'autograd'], default='fused', help='training step: fused C passes or the torch optimiser loop')
    p.add_argument('--dropout', type=float, default=0.5, help='dropout behind every hidden layer')
    p.add_argument('--feed', default='loader', choices=['loader', 'resident'],
                   help="'loader': a DataLoader opens every slide's store every epoch (the reference's feed); 'resident': the cohort is read "
                        "once, kept on the device and every batch is one gather there (same batches, same order, same RNG draws)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from ..he2rna import HE2RNA, fit, he2rna_predict

    seed_everything(args.seed)
    save_dir = os.path.join(args.destfolder, args.subfolder, args.exp_name)
    os.makedirs(save_dir, exist_ok=True)
    if args.log:
        try:
            import wandb
            wandb.init(project="sequoia", config=args, name=args.exp_name)
        except Exception:
            print('wandb not available: logging to stdout only')

    df = pd.read_csv(args.path_csv)
    if args.tcga_projects:
        df = df[df['tcga_project'].isin(args.tcga_projects)]
    df = filter_no_features(df, args.feature_path, 'cluster_features')

    device = "cuda:0"
    table = CohortTable(df, args.feature_path).to(device) if args.feed == 'resident' else None       # one table for every fold and role
    results = {}
    train_idxs, val_idxs, test_idxs = patient_kfold(df, n_splits=args.k)
    for i, (train_idx, val_idx, test_idx) in enumerate(zip(train_idxs, val_idxs, test_idxs)):
        if table is not None:
            train_set = table                                  # feature_dim and num_genes are the cohort's
            train_loader, valid_loader, test_loader = (ResidentLoader(table, idx, args.batch_size, shuffle=shuffle)
                                                       for idx, shuffle in ((train_idx, True), (val_idx, False), (test_idx, False)))
        else:
            train_set, val_set, test_set = (SuperTileRNADataset(df.iloc[idx], args.feature_path) for idx in (train_idx, val_idx, test_idx))
            # the dataset reads small per-slide files; worker processes would each need the library's device context
            train_loader, valid_loader, test_loader = (
                DataLoader(ds, batch_size=args.batch_size, shuffle=shuffle, num_workers=0, collate_fn=custom_collate_fn)
                for ds, shuffle in ((train_set, True), (val_set, False), (test_set, False)))
        model = HE2RNA(input_dim=train_set.feature_dim, layers=LAYERS, ks=KS, dropout=args.dropout, device=device,
                       output_dim=args.num_genes if args.change_num_genes else train_set.num_genes)
        if args.checkpoint:
            model.load_state_dict(torch.load(args.checkpoint, map_location=device, weights_only=False).state_dict())
        if args.change_num_genes:                              # the pretrained head predicts another gene list
            model.replace_head(train_set.num_genes)
        random_preds, _, _, _ = he2rna_predict(model, test_loader)
        preds, labels, wsis, projs = fit(model=model, lr=args.lr, train_loader=train_loader, valid_loader=valid_loader,
                                         test_loader=test_loader, params={'max_epochs': args.max_epochs, 'patience': args.patience},
                                         fold=i, optimizer=None, path=save_dir, engine=args.engine, seed=args.seed)
        results[f'split_{i}'] = {'real': labels, 'preds': preds, 'random': random_preds, 'wsi_file_name': wsis, 'tcga_project': projs}
    results['genes'] = [c[4:] for c in df.columns if 'rna_' in c]
    with open(os.path.join(save_dir, 'test_results.pkl'), 'wb') as f:
        pickle.dump(results, f, protocol=pickle.HIGHEST_PROTOCOL)
    return results, save_dir


if __name__ == '__main__':
    main()
