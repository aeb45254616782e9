function xyzPoints = reconstructScene(disparityMap, reprojectionMatrix, varargin)
%reconstructScene  Dense 3-D scene from a disparity map on the GPU through vo_mex('reconstructscene', ...).
%   xyzPoints = reconstructScene(disparityMap, reprojectionMatrix) shadows the toolbox function of the same
%   name when this folder is ahead of it on the path.  disparityMap is the single map disparitySGM returns;
%   reprojectionMatrix is the 4 x 4 Q with [X Y Z W]' = Q * [x y d 1]' (x = column, y = row, 1-based), as
%   vo_reprojection_matrix builds it from the pair's projection matrices.  xyzPoints is rows x cols x 3 single,
%   NaN where the disparity is NaN (DESIGN.md 3.5.5).  The toolbox's function has no options; anything more is
%   refused by name.
if ~isempty(varargin)
    name = varargin{1};
    if ~(ischar(name) || isstring(name)), name = class(name); end
    error('vo:reconstructScene:options', 'reconstructScene: unsupported argument %s', char(name));
end
if ~isa(disparityMap, 'single'), disparityMap = single(disparityMap); end
xyz = vo_mex('reconstructscene', disparityMap, double(reprojectionMatrix));
xyzPoints = reshape(xyz, size(disparityMap, 1), size(disparityMap, 2), 3);
end
