"""`gfd.nn`: blocks, MuS-GNN, gMuS-GNN and REMuS-GNN models, the GNN base with the rollout loop."""
from . import blocks
from .mus_gnn import *
from .mugs_gnn import NsTwoGuillardScaleGNN, NsThreeGuillardScaleGNN, NsFourGuillardScaleGNN
from .remus_gnn import NsRotEquiTreeScaleGNN
from .model import GNN, TrainConfig, collate, Rollout, RolloutErrors, RolloutMoments, RolloutDerived, RolloutSpectrum, RolloutSamples, RolloutForces, RolloutIntegrals, Spectrum, RolloutWelch, Welch
from ..tracers import RolloutTracers
from ..modes import Modes, SnapshotModes, DynamicModes
from .losses import FlowLoss, ForceLoss, GraphLoss, IntegralLoss, ResidualLoss, SampleLoss
