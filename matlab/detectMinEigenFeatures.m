function points = detectMinEigenFeatures(I, varargin)
%detectMinEigenFeatures  Shi-Tomasi corners on the GPU through vo_mex('corners', ...).
%   points = detectMinEigenFeatures(I, MinQuality = q, FilterSize = f, ROI = [x y w h]) shadows the toolbox
%   function of the same name when this folder is ahead of it on the path and returns
%   cornerPoints(Location, "Metric", Metric).  I is a uint8 grey image (another class is converted with
%   im2uint8).  The spec is libvo's (DESIGN.md 3.5.4): corners come ascending in (row, column), Metric is the
%   pixel's response in the units of a [0, 1] image; points.selectStrongest(N) works on the result as usual.
p = inputParser;
addParameter(p, 'MinQuality', 0.01, @(v) isscalar(v) && isreal(v));
addParameter(p, 'FilterSize', 5, @(v) isscalar(v) && isreal(v));
addParameter(p, 'ROI', [0 0 0 0], @(v) isnumeric(v) && numel(v) == 4);
parse(p, varargin{:});
if ~isa(I, 'uint8'), I = im2uint8(I); end
roi = double(p.Results.ROI(:)');
opts = [0, double(p.Results.FilterSize), double(p.Results.MinQuality), 0, roi];
[Location, Metric] = vo_mex('corners', I, opts);
points = cornerPoints(Location, "Metric", Metric);
end
