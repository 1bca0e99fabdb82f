"""Experiment driver — mirrors `/root/reference/src/experiment.py:29-318`.

Same CLI (``-c/--config``, ``-e/--experiments``, ``--exp_name``), same YAML inputs
(``config.yaml`` + ``experiments.yaml`` / ``econfigs/*.yaml`` with ``grid:`` and ``linear:``
sections), same resolution of model / loader classes from name strings, same per-experiment
catch-and-continue.  Differences, all forced by scope:

* tracking goes to a JSON-lines run log instead of MLflow (not installed);
* ``Model.fit`` is the HIP training step of training.py (every model class named in ``econfigs/`` and the TwoStep / TwoWay
  classes the factories generate); a model or reduction without a training recipe raises and the experiment fails — the
  grid goes on with the next one, nothing is evaluated on untrained weights;
* Precision/Recall/F1@k come from a host-side restatement of RiVal's holdout metrics instead of ``binaries/mimir.jar``
  (utilities/metrics.py: hand-computed vectors in tests/test_metrics_cpu.py).

Run from the directory that holds ``config.yaml`` and the ``datasets/`` tree:
``python -m deep_cbrs_amar_renaissance_amd.experiment -e econfigs/basic-gnn.yaml``
(or ``python src/experiment.py ...`` through the thin ``src/`` shim).
"""
import argparse
import copy
import inspect
import io
import os
import re
import time
import traceback
from os.path import join as path_join
from time import strftime

import numpy as np
import pandas as pd
import yaml

from deep_cbrs_amar_renaissance_amd import engine, models as models_pkg
from deep_cbrs_amar_renaissance_amd.data import loaders
from deep_cbrs_amar_renaissance_amd.data.datasets import holdout_split
from deep_cbrs_amar_renaissance_amd.models.basic import BasicRS, BasicGNN, BasicKnowledgeGCN, BasicTSGNN, BasicTWGNN
from deep_cbrs_amar_renaissance_amd.models.hybrid import HybridCBRS, HybridBertGNN
from deep_cbrs_amar_renaissance_amd.utilities import losses
from deep_cbrs_amar_renaissance_amd.utilities.keras import Callback, EarlyStopping, ReduceLROnPlateau, get_total_parameters
from deep_cbrs_amar_renaissance_amd.utilities.metrics import check_rank_metrics, explanations_frame, full_ranking_metrics, recommendations_frame, resolve_compiled, \
    top_k_predictions, top_k_metrics
from deep_cbrs_amar_renaissance_amd.utilities.schedules import resolve as resolve_learning_rate
from deep_cbrs_amar_renaissance_amd.utilities.utils import \
    get_experiment_logger, nested_dict_update, make_grid, mlflow_linearize, setup_mlflow

PARAMS_PATH = 'config.yaml'
EXPERIMENTS_PATH = 'experiments.yaml'
MLFLOW_PATH = './mlruns'
MLFLOW_EXP_NAME = 'SIS - Movielens-1M - BasicRS with Knowledge GNNs'
LOG_FREQUENCY = 100
METRICS_TOP_KS = [5, 10]

parser = argparse.ArgumentParser()
parser.add_argument("-c", "--config", dest='config', type=str, help="Config input file", default=PARAMS_PATH)
parser.add_argument("-e", "--experiments", dest='experiments', type=str,
                    help="Experiment (grid search) file", default=EXPERIMENTS_PATH)
parser.add_argument("--exp_name", dest='exp_name', type=str,
                    help="Name of the group of runs (used in the run log)", default=MLFLOW_EXP_NAME)


class _Yaml12Loader(yaml.SafeLoader):
    """PyYAML is YAML 1.1: '1e-4' (no dot) would load as a string. The reference reads its configs
    with ruamel (YAML 1.2), where it is a float — resolve floats the 1.2 way."""


_Yaml12Loader.add_implicit_resolver(
    'tag:yaml.org,2002:float',
    re.compile(r'^[-+]?(\.[0-9]+|[0-9]+(\.[0-9]*)?)([eE][-+]?[0-9]+)?$|^[-+]?\.(inf|Inf|INF)$|^\.(nan|NaN|NAN)$'),
    list('-+0123456789.'))


def load_yaml(path):
    with open(path, 'r') as fp:
        return yaml.load(fp, Loader=_Yaml12Loader)


class AttrDict(dict):
    """dict with attribute access, nested (the reference uses EasyDict)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    def __setitem__(self, key, value):
        if isinstance(value, dict) and not isinstance(value, AttrDict):
            value = AttrDict(value)
        super().__setitem__(key, value)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    __setattr__ = __setitem__


def _store_clip(optimizer, clipnorm, clipvalue, global_clipnorm):
    """The gradient clip of every Keras 2 optimizer as attributes of `optimizer`: only what is set (None = off reads back as None through
    the class attributes below), so an optimizer without a clip carries its hyper-parameters alone."""
    for name, value in (('clipnorm', clipnorm), ('clipvalue', clipvalue), ('global_clipnorm', global_clipnorm)):
        if value is not None:
            setattr(optimizer, name, value)


def _store_rate(optimizer, learning_rate, decay):
    """`learning_rate` as a number or a schedule (utilities/schedules.py:resolve — an object, an experiment file's mapping {name: ...} or
    Keras' {class_name, config}) and Keras 2's `decay`, the rate lr / (1 + decay * step), kept as an attribute only where it is set.
    Refused here, where the optimizer is built, by training.OptimizerSpec's rule: what is no rate, a negative decay, a decay together
    with a schedule.  OptimizerSpec turns the two into the schedule the device follows."""
    from deep_cbrs_amar_renaissance_amd.training import OptimizerSpec
    optimizer.learning_rate = resolve_learning_rate(learning_rate)
    if decay is not None:
        optimizer.decay = decay
    OptimizerSpec._checked_schedule(optimizer.learning_rate, decay)


class Adam:
    """keras.optimizers.Adam's constructor (config.yaml:52-56); amsgrad=True selects the AMSGrad rule.  The optimizer classes only carry
    their rule, hyper-parameters and gradient clip (clipnorm / clipvalue / global_clipnorm, named in every signature so that
    Experimenter.build_optimizer's filter lets them through; training.OptimizerSpec validates them): training.py keeps the state and runs
    the clip and the update on the device."""
    rule = 'Adam'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon, self.amsgrad = learning_rate, beta_1, beta_2, epsilon, bool(amsgrad)
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)
        if self.amsgrad:
            self.rule = 'AMSGrad'


class SGD:
    rule = 'SGD'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.momentum, self.nesterov = learning_rate, momentum, bool(nesterov)
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)


class RMSprop:
    rule = 'RMSprop'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.rho, self.momentum, self.epsilon, self.centered = learning_rate, rho, momentum, epsilon, bool(centered)
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)


class Adagrad:
    rule = 'Adagrad'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7,
                 clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.initial_accumulator_value, self.epsilon = learning_rate, initial_accumulator_value, epsilon
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)


class Adamax:
    rule = 'Adamax'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)


class Nadam:
    rule = 'Nadam'
    clipnorm = clipvalue = global_clipnorm = decay = None

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clipvalue=None, global_clipnorm=None, decay=None, **kwargs):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon
        _store_clip(self, clipnorm, clipvalue, global_clipnorm)
        _store_rate(self, learning_rate, decay)


OPTIMIZERS = {cls.__name__: cls for cls in (Adam, SGD, RMSprop, Adagrad, Adamax, Nadam)}


def optimizer_class(name):
    """`getattr(tf.keras.optimizers, name)` of the reference (src/experiment.py:111) for the rules that train on the device."""
    if name not in OPTIMIZERS:
        raise ValueError("optimizer '{}' is not supported: choose one of {} (Adam takes amsgrad: True)".format(name, ', '.join(sorted(OPTIMIZERS))))
    return OPTIMIZERS[name]


class RunLogCallback(Callback):
    """The reference's LogCallback (utilities/keras.py there) for fit(): every epoch's logs go to the run log with step = epoch, and
    the end of training logs where an EarlyStopping stopped and which epoch was best."""

    def __init__(self, run_log, stopping=None):
        self.run_log, self.stopping = run_log, stopping

    def on_epoch_end(self, epoch, logs=None):
        self.run_log.log_metrics({name: float(value) for name, value in (logs or {}).items()}, step=epoch)

    def on_train_end(self, logs=None):
        if self.stopping is not None:
            self.run_log.log_metrics({'stopped_epoch': int(self.stopping.stopped_epoch), 'best_epoch': int(self.stopping.best_epoch)})


class Experimenter:
    def __init__(self, config, run_log):
        """Holds every object of one experiment and performs its training and evaluation."""
        self.run_log = run_log
        self.config = AttrDict(copy.deepcopy(config))
        engine.set_seed(self.config.seed)

        self.exp_name = strftime("%m_%d-%H_%M") + '-' + self.config.model.name
        if BasicRS.__name__ in self.config.model.name:
            pass
        elif HybridCBRS.__name__ in self.config.model.name:
            self.exp_name += '-' + ('feature' if self.config.model.feature_based else 'entity')
        else:
            self.exp_name += '-' + str(self.config.model.l2_regularizer) + '-' + self.config.model.final_node
        if self.config.get('details'):
            self.exp_name += '-' + self.config.details
        run_log.start_run(run_name=self.exp_name)
        run_log.log_params(mlflow_linearize(config))

        self.config.dest = path_join(run_log.run_dir, 'artifacts')
        self.predictions_dest = path_join(self.config.dest, "predictions")
        os.makedirs(self.predictions_dest, exist_ok=True)
        with open(path_join(self.config.dest, "config.yaml"), 'w') as fp:       # reproducibility copy
            yaml.safe_dump(config, fp)

        self.logger = get_experiment_logger(self.config.dest)
        buf = io.StringIO()
        yaml.safe_dump(config, buf)
        self.logger.info('CONFIG')
        self.logger.info(buf.getvalue())

        self._retrieve_classes()
        self.trainset = self.testset = self.model = self.optimizer = None
        self.parameters = self.config.parameters

    def _retrieve_classes(self):
        """Object classes from name strings (experiment.py:107-118)."""
        self.optimizer_class = optimizer_class(self.config.parameters.optimizer.name)
        model_module, model_class = self.config.model.name.split('.')
        module = __import__(models_pkg.__name__ + '.' + model_module, fromlist=[model_class])
        self.model_class = getattr(module, model_class)
        self.load_function = getattr(loaders, self.config.dataset.load_function_name)

    def build_dataset(self):
        accepted = inspect.signature(self.load_function).parameters
        kwargs = {k: self.config.dataset[k] for k in self.config.dataset.keys() & accepted.keys()}
        self.valset = None
        validation = self.config.parameters.get('validation')
        if validation:
            # parameters.validation: a share of the training rows is held out (datasets.holdout_split, seeded with config.seed) and both
            # parts are written next to the run's other artifacts; the kept part is the training file of this run, so the graph holds
            # no held-out edge, and the held-out part is read through the same load function as a test file
            sep = kwargs.get('sep', '\t')
            raw = pd.read_csv(kwargs['train_ratings_filepath'], sep=sep, header=None)
            kept, held = holdout_split(raw.to_numpy(), float(validation.get('fraction', 0.1)), self.config.seed)
            dest = path_join(self.config.dest, 'validation')
            os.makedirs(dest, exist_ok=True)
            kept_path, held_path = path_join(dest, 'train_kept.tsv'), path_join(dest, 'validation.tsv')
            for part, path in ((kept, kept_path), (held, held_path)):
                pd.DataFrame(part).astype(raw.dtypes.to_dict()).to_csv(path, sep=sep, header=False, index=False)
            kwargs['train_ratings_filepath'] = kept_path
            _, self.valset = self.load_function(**dict(kwargs, test_ratings_filepath=held_path))
        self.trainset, self.testset = self.load_function(**kwargs)
        # the loaders index the properties and drop their original identifiers: explanations are written with them
        self.property_ids = None
        if kwargs.get('props_triples_filepath') and kwargs.get('type_adjacency') in ('unary-uip', 'unary-kg'):
            self.property_ids = loaders.property_identifiers(kwargs['props_triples_filepath'], kwargs.get('sep', '\t'))

    def validation_fit_args(self):
        """fit()'s validation arguments from parameters.validation ({fraction, freq, ranking_ks, full_ranking_rank_metrics,
        early_stopping, reduce_lr}); {} without the key."""
        validation = self.config.parameters.get('validation')
        if not validation:
            return {}
        callbacks = []
        stopping = None
        if validation.get('early_stopping'):
            stopping = EarlyStopping(**dict(validation.get('early_stopping')))
            callbacks.append(stopping)
        if validation.get('reduce_lr'):                              # {monitor, factor, patience, cooldown, min_lr, min_delta}
            callbacks.append(ReduceLROnPlateau(**dict(validation.get('reduce_lr'))))
        callbacks.append(RunLogCallback(self.run_log, stopping))     # (last: it logs what the others added, `lr` among it)
        args = {'validation_data': self.valset, 'validation_freq': int(validation.get('freq', 1)), 'callbacks': callbacks}
        if validation.get('ranking_ks') or validation.get('full_ranking_rank_metrics'):
            args['validation_ranking'] = {'trainset': self.trainset, 'ratings': self.valset.ratings,
                                          'ks': [int(k) for k in validation.get('ranking_ks') or []], 'users': None}
            if validation.get('full_ranking_rank_metrics'):          # val_auc / val_mrr / val_map per validated epoch
                args['validation_ranking']['rank_metrics'] = check_rank_metrics(validation.get('full_ranking_rank_metrics'))
        return args

    def class_weight(self):
        """fit()'s class_weight from parameters.class_weight — a mapping over the classes 0 and 1 (YAML's string keys included) or
        `balanced` — resolved against the labels of the training rows (after the validation split, where there is one) and logged as
        the parameters class_weight.0 / class_weight.1; None without the key."""
        pair = losses.resolve_class_weight(self.parameters.get('class_weight'), np.asarray(self.trainset.ratings)[:, 2])
        if pair is not None:
            self.run_log.log_params({'class_weight.0': pair[0], 'class_weight.1': pair[1]})
        return pair

    def build_optimizer(self):
        accepted = inspect.signature(self.optimizer_class).parameters
        opt_cfg = self.config.parameters.optimizer
        self.optimizer = self.optimizer_class(**{k: opt_cfg[k] for k in opt_cfg.keys() & accepted.keys()})

    def build_model(self):
        self.logger.info('Building model...')
        cls, model_cfg = self.model_class, dict(self.config.model)
        if issubclass(cls, (BasicKnowledgeGCN, BasicTSGNN, BasicTWGNN)):
            self.model = cls(len(self.trainset.users), len(self.trainset.items), self.trainset.adj_matrix, **model_cfg)
        elif issubclass(cls, (BasicGNN, HybridBertGNN)):
            self.model = cls(self.trainset.adj_matrix, **model_cfg)
        else:
            self.model = cls(**model_cfg)
        if hasattr(self.model, 'n_users'):                   # lets hoisted scoring run each tower on its own rows
            self.model.n_users, self.model.n_items = len(self.trainset.users), len(self.trainset.items)
        # custom loss class (experiment.py:155-157: BPRLoss and the listwise losses, with their defaults); any other name, or a
        # mapping {name: ..., <hyper-parameters>} such as {name: SampledSoftmaxLoss, temperature: 0.2}, goes to compile()
        custom = getattr(losses, self.parameters.loss, None) if isinstance(self.parameters.loss, str) else None
        if isinstance(custom, type) and custom.__module__ == losses.__name__:
            self.parameters['loss'] = custom()
        self.model.compile(loss=self.parameters.loss, optimizer=self.optimizer, metrics=self.parameters.metrics)
        self.model(self.trainset[0][0])                       # one prediction builds every weight
        self.model.summary(print_fn=self.logger.info, expand_nested=True)
        trainable, non_trainable = get_total_parameters(self.model)
        self.run_log.log_metrics({'trainable_params': trainable, 'non_trainable_params': non_trainable})

    def train(self):
        self.logger.info("Experiment folder: " + self.config.dest)
        if self.config.parameters.get('full_ranking_rank_metrics'):  # an unknown name fails here, not after the training
            check_rank_metrics(self.config.parameters.get('full_ranking_rank_metrics'))
        self.build_dataset()
        self.build_optimizer()
        self.build_model()
        self.logger.info('Training:')
        t0 = time.perf_counter()
        # a model or reduction without a training recipe raises here: the experiment fails (MultiExperimenter.run_experiment
        # logs the traceback, ends the run and goes on with the grid, experiment.py:295-302) instead of evaluating random weights
        self.model.fit(self.trainset, epochs=self.parameters.epochs, workers=self.config.n_workers, class_weight=self.class_weight(),
                       **self.validation_fit_args())
        # the reference's LogCallback reports the fit wall time as 'training_time' (utilities/keras.py:43-51, 69-85)
        self.run_log.log_metrics({'training_time': time.perf_counter() - t0})

    def evaluate(self):
        loss_acc = self.model.evaluate(self.testset)
        # evaluate(): [loss, accuracy] when no metric or only accuracy is compiled, else [loss, <metrics in compile order>]
        names = resolve_compiled(self.model.loss, self.model.metrics)[2]
        if all(name == 'accuracy' for name in names):
            self.run_log.log_metrics({'test_loss': loss_acc[0], 'test_accuracy': loss_acc[1]})
        else:
            self.run_log.log_metrics(dict({'test_loss': loss_acc[0]}, **{'test_' + name: v for name, v in zip(names, loss_acc[1:])}))
        predictions = self.model.predict(self.testset)
        ratings_pred = np.concatenate([self.testset.ratings[:, [0, 1]], predictions], axis=1)
        precision_at, recall_at, f1_at = {}, {}, {}
        for k in METRICS_TOP_KS:
            top_predictions = top_k_predictions(ratings_pred, self.trainset.users, self.trainset.items, k=k)
            top_k_dest = path_join(self.predictions_dest, "top_{}".format(k))
            os.makedirs(top_k_dest, exist_ok=True)
            top_predictions.to_csv(path_join(top_k_dest, "predictions_1.tsv"), sep='\t', header=False, index=False)
            # the evaluator's switches are reachable from the experiment config (parameters.metrics_short_lists / metrics_no_relevant);
            # unset = RiVal's behaviour as restated (utilities/metrics.py), users skipped by them are logged with the metrics
            prm = self.config.parameters
            top_k_metrics(self.config.dataset.test_ratings_filepath, top_k_dest,
                          short_lists=prm.get('metrics_short_lists'), no_relevant=prm.get('metrics_no_relevant'))
            users_tsv = path_join(top_k_dest, "results_users.tsv")
            if os.path.exists(users_tsv):
                cnt = pd.read_csv(users_tsv, sep='\t').iloc[0]
                self.run_log.log_metrics({"users_skipped_short_list_at_{}".format(k): int(cnt['skipped_short_list']),
                                          "users_skipped_no_relevant_at_{}".format(k): int(cnt['skipped_no_relevant_item'])})
            results = pd.read_csv(path_join(top_k_dest, "results.tsv"), sep='\t', header=None)
            results = results.drop(0, axis=1).to_numpy().squeeze()
            precision_at[k], recall_at[k], f1_at[k] = results[0], results[1], results[2]
            self.run_log.log_metrics({"precision_at_{}".format(k): precision_at[k],
                                      "recall_at_{}".format(k): recall_at[k],
                                      "f1_at_{}".format(k): f1_at[k]})
        metrics = pd.DataFrame([precision_at, recall_at, f1_at], index=['precision_at', 'recall_at', 'f1_at'])
        if self.config.parameters.get('full_ranking_ks'):
            self.evaluate_full_ranking([int(k) for k in self.config.parameters.get('full_ranking_ks')])
        if self.config.parameters.get('full_ranking_rank_metrics'):
            self.evaluate_full_ranking_rank_metrics(self.config.parameters.get('full_ranking_rank_metrics'))
        if self.config.parameters.get('similar_items'):
            self.write_similar_items(**dict(self.config.parameters.get('similar_items')))
        if self.config.parameters.get('diversify'):
            self.write_diverse(**dict(self.config.parameters.get('diversify')))
        if self.config.parameters.get('calibrate'):
            self.write_calibrated(**dict(self.config.parameters.get('calibrate')))
        if self.config.parameters.get('explain'):
            self.write_explanations(**dict(self.config.parameters.get('explain')))
        if self.config.parameters.get('group_recommend'):
            self.write_group_recommend(**dict(self.config.parameters.get('group_recommend')))
        if self.config.parameters.get('recommend_among'):
            self.write_recommend_among(**dict(self.config.parameters.get('recommend_among')))
        if self.config.parameters.get('recommend_deep'):
            self.write_recommend_deep(**dict(self.config.parameters.get('recommend_deep')))
        self.logger.info('\n' + str(metrics))
        print('\n' + str(metrics))
        return metrics

    def evaluate_full_ranking(self, ks):
        """Opt-in (parameters.full_ranking_ks): every user's top-max(ks) among ALL items it has not rated in training
        (`recommend()`), written as <predictions_dest>/full_ranking/top_<k>.tsv (user, item, score; original ids) and scored
        against the test ratings with Precision / Recall / NDCG / HitRate @k (utilities/metrics.py:full_ranking_metrics)."""
        users, items, scores = self.model.recommend(self.trainset, k=max(ks))
        dest = path_join(self.predictions_dest, "full_ranking")
        os.makedirs(dest, exist_ok=True)
        for k in ks:
            recommendations_frame(users, items[:, :k], scores[:, :k], self.trainset.users, self.trainset.items).to_csv(
                path_join(dest, "top_{}.tsv".format(k)), sep='\t', header=False, index=False)
        full = full_ranking_metrics(users, items, self.testset.ratings, ks)
        self.run_log.log_metrics({'full_' + name: value for name, value in full.items()
                                  if name not in ('users_evaluated', 'users_skipped')})
        self.run_log.log_metrics({'full_ranking_users_evaluated': full['users_evaluated'],
                                  'full_ranking_users_skipped': full['users_skipped']})
        return full

    def evaluate_full_ranking_rank_metrics(self, names):
        """Opt-in (parameters.full_ranking_rank_metrics: [auc, mrr, map] or a subset): the cut-off-free measures of the full ranking —
        the exact rank of every relevant test item among ALL items its user has not rated in training (`evaluate_ranking(rank_metrics=...)`)
        — logged as full_auc / full_mrr / full_map beside the `full_ranking_ks` metrics.  An unknown name is a ValueError."""
        names = check_rank_metrics(names)
        found = self.model.evaluate_ranking(self.trainset, self.testset.ratings, [], rank_metrics=names)
        evaluated, skipped = found.pop('rank_metrics_users')
        self.run_log.log_metrics({'full_' + name: value for name, value in found.items()})
        self.run_log.log_metrics({'full_rank_metrics_users_evaluated': evaluated, 'full_rank_metrics_users_skipped': skipped})
        return found

    def write_similar_items(self, k=10, metric='cosine', space=None):
        """Opt-in (parameters.similar_items: {k, metric, space}): every item's k most similar items in the trained model's `space`
        (`similar_items()`), written as <predictions_dest>/similar_items_<k>.tsv (item, neighbour, score; original ids)."""
        items, neighbours, scores = self.model.similar_items(self.trainset, k=int(k), metric=metric, space=space)
        n_users, item_ids = len(self.trainset.users), self.trainset.items
        # recommendations_frame names its first column through the ids it is given: here the items' own, for both columns
        frame = recommendations_frame(items - n_users, np.where(neighbours >= 0, neighbours - n_users + len(item_ids), -1), scores,
                                      item_ids, item_ids)
        path = path_join(self.predictions_dest, "similar_items_{}.tsv".format(int(k)))
        frame.to_csv(path, sep='\t', header=False, index=False)
        return path

    def write_diverse(self, k=10, pool=50, trade_off=0.7, metric='cosine', space=None):
        """Opt-in (parameters.diversify: {k, pool, trade_off, metric, space}): every user's `pool` best unseen items re-ranked by
        Maximal Marginal Relevance (`recommend_diverse()`), written as <predictions_dest>/diverse_top_<k>.tsv (user, item, score;
        original ids, selection order); the intra-list diversity and the catalogue coverage at k of the plain top-k and of the
        diversified lists are logged as plain_ / diverse_ ild_at_<k> and item_coverage_at_<k>."""
        import torch
        from deep_cbrs_amar_renaissance_amd import recommend as rec
        k = int(k)
        users, items, scores = self.model.recommend_diverse(self.trainset, k=k, pool=int(pool), trade_off=float(trade_off),
                                                            metric=metric, space=space)
        path = path_join(self.predictions_dest, "diverse_top_{}.tsv".format(k))
        recommendations_frame(users, items, scores, self.trainset.users, self.trainset.items).to_csv(
            path, sep='\t', header=False, index=False)
        n_users, n_items = len(self.trainset.users), len(self.trainset.items)
        table = self.model._item_embeddings(self.trainset, space)
        with rec.device_lists():
            _, plain, _ = self.model.recommend(self.trainset, k=k)
        diverse = torch.from_numpy(np.where(items >= 0, items - n_users, -1).astype(np.int32)).to(table.device)
        logged = {}
        for prefix, lists in (('plain_', plain.contiguous()), ('diverse_', diverse)):
            if len(users):
                logged.update({prefix + name: value for name, value in rec.diversity_metrics(lists, table, [k], metric, n_items).items()})
        self.run_log.log_metrics(logged)
        return path, logged

    def write_calibrated(self, k=10, pool=50, trade_off=0.5, smoothing=0.01, categories=None):
        """Opt-in (parameters.calibrate: {k, pool, trade_off, smoothing, categories}; categories null or an int): every user's `pool`
        best unseen items re-ranked towards the categories of what the user liked (`recommend_calibrated()`), written as
        <predictions_dest>/calibrated_top_<k>.tsv (user, item, score; original ids, selection order); the miscalibration at k of the
        plain top-k and of the calibrated lists is logged as plain_ / calibrated_miscalibration_at_<k>."""
        import torch
        from deep_cbrs_amar_renaissance_amd import recommend as rec
        k = int(k)
        if categories is not None and (isinstance(categories, bool) or not isinstance(categories, int)):
            raise ValueError("parameters.calibrate.categories must be null or an integer (got {!r})".format(categories))
        users, items, scores = self.model.recommend_calibrated(self.trainset, k=k, pool=int(pool), trade_off=float(trade_off),
                                                               smoothing=float(smoothing), categories=categories)
        path = path_join(self.predictions_dest, "calibrated_top_{}.tsv".format(k))
        recommendations_frame(users, items, scores, self.trainset.users, self.trainset.items).to_csv(
            path, sep='\t', header=False, index=False)
        n_users, n_items = len(self.trainset.users), len(self.trainset.items)
        logged = {}
        if len(users):
            with rec.device_lists():
                _, plain, _ = self.model.recommend(self.trainset, k=k)
            calibrated = torch.from_numpy(np.where(items >= 0, items - n_users, -1).astype(np.int32)).to(plain.device)
            liked, cats = rec._liked_device(self.trainset, n_users, n_items), rec._cats_device(self.trainset, n_items, categories)
            for prefix, lists in (('plain_', plain.contiguous()), ('calibrated_', calibrated)):
                logged.update({prefix + name: value for name, value in rec.calibration_metrics(lists, None, liked, cats, [k], smoothing).items()})
        self.run_log.log_metrics(logged)
        return path, logged

    def write_explanations(self, k=10, n_evidence=3, n_properties=3, metric='cosine', space=None):
        """Opt-in (parameters.explain: {k, n_evidence, n_properties, metric, space}): every user's top-k explained (`explain()`),
        written as <predictions_dest>/explanations_<k>.tsv, one row per (user, item, rank): user, item, rank, evidence items,
        their similarities, shared properties, their scores, their supports (lists joined by spaces; original identifiers, the
        properties by the loader's identifiers or, for a trainset that came without them, by property index)."""
        out = self.model.explain(self.trainset, k=int(k), n_evidence=int(n_evidence), n_properties=int(n_properties), metric=metric,
                                 space=space)
        path = path_join(self.predictions_dest, "explanations_{}.tsv".format(int(k)))
        explanations_frame(out, self.trainset.users, self.trainset.items, getattr(self, 'property_ids', None)).to_csv(
            path, sep='\t', header=False, index=False)
        return path

    def group_members(self, groups):
        """The groups of parameters.group_recommend.groups as (group ids, list of user-index arrays): a path to a two-column TSV
        (group id, original user id; users that are not in the training set are dropped with a log line, groups in order of first
        appearance) or {size, count, seed}: `count` random groups of `size` distinct training users from
        numpy.random.default_rng(seed)."""
        n_users = len(self.trainset.users)
        if isinstance(groups, str):
            frame = pd.read_csv(groups, sep='\t', header=None, usecols=[0, 1])
            index = {u: r for r, u in enumerate(np.asarray(self.trainset.users).tolist())}
            rows = frame[1].map(index)
            if rows.isna().any():
                self.logger.info("group_recommend: {} of {} listed users are not in the training set: dropped".format(
                    int(rows.isna().sum()), len(frame)))
            frame = frame.assign(row=rows)[rows.notna()]
            ids = list(dict.fromkeys(frame[0].tolist()))
            return ids, [np.unique(frame['row'][frame[0] == gid].astype(np.int64).to_numpy()) for gid in ids]
        size, count = int(groups['size']), int(groups['count'])
        if not 1 <= size <= n_users or count < 0:
            raise ValueError("group_recommend.groups: size must lie in [1, {}] and count must not be negative".format(n_users))
        rng = np.random.default_rng(int(groups.get('seed', 0)))
        return list(range(count)), [rng.choice(n_users, size=size, replace=False).astype(np.int64) for _ in range(count)]

    def write_group_recommend(self, k=10, strategy='mean', min_score=None, groups=None):
        """Opt-in (parameters.group_recommend: {k, strategy, min_score, groups}): the k best unseen items of every group
        (`recommend_group()`; `groups` as `group_members` reads them), written as <predictions_dest>/group_top_<k>.tsv, one row
        per (group, rank): group, rank, item (original id), score."""
        if groups is None:
            raise ValueError("parameters.group_recommend needs `groups`: a TSV path or {size, count, seed}")
        k = int(k)
        ids, members = self.group_members(groups)
        items, scores = self.model.recommend_group(self.trainset, members, k=k, strategy=strategy,
                                                   min_score=None if min_score is None else float(min_score))
        n_users, item_ids = len(self.trainset.users), np.asarray(self.trainset.items)
        g, r = np.nonzero(items >= 0)
        frame = pd.DataFrame({'group': np.asarray(ids, dtype=object)[g] if len(ids) else [], 'rank': r + 1,
                              'item': item_ids[items[g, r] - n_users], 'score': scores[g, r]})
        path = path_join(self.predictions_dest, "group_top_{}.tsv".format(k))
        frame.to_csv(path, sep='\t', header=False, index=False)
        return path

    def write_recommend_among(self, k=10, candidates=None, any_of=None, all_of=None, none_of=None):
        """Opt-in (parameters.recommend_among: {k, candidates: [...]} or {k, any_of / all_of / none_of: [...]}): every user's k best
        unseen items among a candidate set (`recommend_among()`), written as <predictions_dest>/among_top_<k>.tsv, one row per
        (user, rank): user (original id), rank, item (original id), score.  `candidates` lists ORIGINAL item ids (those that are not
        in the training set are dropped with a log line); the property filters take property indices as `items_with_properties`
        does and are used when `candidates` is absent."""
        from deep_cbrs_amar_renaissance_amd.recommend import items_with_properties
        k = int(k)
        n_users, item_ids = len(self.trainset.users), np.asarray(self.trainset.items)
        if candidates is not None:
            if any_of is not None or all_of is not None or none_of is not None:
                raise ValueError("parameters.recommend_among takes `candidates` or the property filters, not both")
            index = {i: r for r, i in enumerate(item_ids.tolist())}
            rows = [index[c] for c in list(candidates) if c in index]
            if len(rows) != len(list(candidates)):
                self.logger.info("recommend_among: {} of {} listed items are not in the training set: dropped".format(
                    len(list(candidates)) - len(rows), len(list(candidates))))
            chosen = np.asarray(rows, dtype=np.int64) + n_users
        elif any_of is None and all_of is None and none_of is None:
            raise ValueError("parameters.recommend_among needs `candidates` (item ids) or one of any_of / all_of / none_of (property indices)")
        else:
            chosen = items_with_properties(self.trainset, any_of=any_of, all_of=all_of, none_of=none_of)
        users, items, scores = self.model.recommend_among(self.trainset, chosen, k=k)
        u, r = np.nonzero(items >= 0)
        frame = pd.DataFrame({'user': np.asarray(self.trainset.users)[users[u]] if len(users) else [], 'rank': r + 1,
                              'item': item_ids[items[u, r] - n_users], 'score': scores[u, r]})
        path = path_join(self.predictions_dest, "among_top_{}.tsv".format(k))
        frame.to_csv(path, sep='\t', header=False, index=False)
        return path

    def write_recommend_deep(self, k=100):
        """Opt-in (parameters.recommend_deep: {k}): every user's first k unseen items for k up to 1024 (`recommend_deep()`: chained
        pages past the 64 of one `recommend()` call), written as <predictions_dest>/deep_top_<k>.tsv (user, item, score; original ids)."""
        k = int(k)
        users, items, scores = self.model.recommend_deep(self.trainset, k=k)
        path = path_join(self.predictions_dest, "deep_top_{}.tsv".format(k))
        recommendations_frame(users, items, scores, self.trainset.users, self.trainset.items).to_csv(
            path, sep='\t', header=False, index=False)
        return path

    def run(self):
        self.train()
        metrics = self.evaluate()
        self.close()
        return metrics

    def close(self):
        for handler in list(self.logger.handlers):
            handler.close()
            self.logger.removeHandler(handler)
        self.run_log.end_run()


class MultiExperimenter:
    """Runs every experiment of an experiments file, each as overrides on the base config."""

    def __init__(self, params_path, experiments_path, run_log):
        self.run_log = run_log
        self.base_config = load_yaml(params_path)
        config = load_yaml(experiments_path) or {}
        self.experiments = dict(config.get('linear') or {})
        for grid in (config.get('grid') or {}).values():
            self.experiments.update({str(elem): elem for elem in make_grid(grid)})
        print("Retrieved experiments: {}".format(len(self.experiments)))
        for exp in self.experiments:
            print(exp)

    def run_experiment(self, exp_name):
        overrides = self.experiments[exp_name]
        config = copy.deepcopy(self.base_config)
        if overrides:                                        # None runs the base config
            config = nested_dict_update(config, overrides)
        print('-----------------------------------------------\n{}\n'.format(exp_name),
              '-----------------------------------------------\n')
        try:
            return Experimenter(config, self.run_log).run()
        except Exception as e:                               # keep going with the rest of the grid
            print(e)
            traceback.print_exc()
            self.run_log.end_run()
            return None

    def run(self):
        n_exp = len(self.experiments)
        results = {}
        for i, exp_name in enumerate(self.experiments):
            print("Experiment {}/{}".format(i + 1, n_exp))
            results[exp_name] = self.run_experiment(exp_name)
        return results


def main(argv=None):
    args = parser.parse_args(argv)
    run_log = setup_mlflow(args.exp_name, MLFLOW_PATH)
    MultiExperimenter(args.config, args.experiments, run_log).run()


if __name__ == "__main__":
    main()
