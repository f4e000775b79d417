"""AverageMeter (reference: src/lib/utils/utils.py)."""


class AverageMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        if self.count > 0:
            self.avg = self.sum / self.count


class BestMetric(object):
    """The rule that picks model_best.pth (main.py): a validation loss statistic wins when it is lower than the best
    so far, `ap` when it is higher.  A NaN never wins (every comparison with it is false)."""

    def __init__(self, metric):
        self.higher = metric == "ap"
        self.best = float("-inf") if self.higher else 1e10

    def update(self, value):
        """True when `value` is the new best."""
        better = value > self.best if self.higher else value < self.best
        if better:
            self.best = value
        return bool(better)
