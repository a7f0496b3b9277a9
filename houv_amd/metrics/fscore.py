"""F-score of two clouds (utils/metrics/CD/fscore.py:3-16)."""
import torch


def fscore(dist1, dist2, threshold=0.0001):
    """dist1[B,N], dist2[B,M]: SQUARED nearest-neighbour distances (adapt the threshold accordingly).
    Returns (fscore, precision_1, precision_2), each [B]; the F-score is 0 where both precisions are 0."""
    precision_1 = torch.mean((dist1 < threshold).float(), dim=1)
    precision_2 = torch.mean((dist2 < threshold).float(), dim=1)
    fscore = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    fscore[torch.isnan(fscore)] = 0
    return fscore, precision_1, precision_2
