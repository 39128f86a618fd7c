"""LeNet of the reference's CIFAR run (Man_Colab.ipynb cell 19, ``model_name = 'lenet'``; the
submodule's networks/lenet.py): two 5 x 5 convolutions with ReLU and 2 x 2 max-pooling, then
400 -> 120 -> 84 -> num_classes.  Parameter registration order (conv1.w, conv1.b, ..., fc3.b) is
the flatten order ``Mixer`` uses (mixer.py:69), the layout of a row of ``dl_lenet_grad``."""
import torch.nn as nn
import torch.nn.functional as F


class LeNet(nn.Module):
    def __init__(self, num_classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 6, 5)
        self.conv2 = nn.Conv2d(6, 16, 5)
        self.fc1 = nn.Linear(16 * 5 * 5, 120)
        self.fc2 = nn.Linear(120, 84)
        self.fc3 = nn.Linear(84, num_classes)

    def forward(self, x):
        out = F.max_pool2d(F.relu(self.conv1(x)), 2)
        out = F.max_pool2d(F.relu(self.conv2(out)), 2)
        out = out.view(out.size(0), -1)
        out = F.relu(self.fc1(out))
        out = F.relu(self.fc2(out))
        return self.fc3(out)

    @staticmethod
    def param_shapes(num_classes=10):
        """Flattened-row layout: [(name, shape)] in registration order."""
        return [("conv1.weight", (6, 3, 5, 5)), ("conv1.bias", (6,)),
                ("conv2.weight", (16, 6, 5, 5)), ("conv2.bias", (16,)),
                ("fc1.weight", (120, 400)), ("fc1.bias", (120,)),
                ("fc2.weight", (84, 120)), ("fc2.bias", (84,)),
                ("fc3.weight", (num_classes, 84)), ("fc3.bias", (num_classes,))]
